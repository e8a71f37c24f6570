"""Scenes, shapes and cases for the seams of the camera physics (csrc/ycge_camera_physics.h, k_camera_tick and k_bodies_tick in
csrc/ycge_camera.hip): bodies that sit exactly on - or within an ulp of - the constants the stepper compares against, walls exactly at a
ray's tMax, rays that tie, headings along the lattice: the decisions no body of tests/volume_camera_cases.py's drawn sequences reaches.
numpy and the package's scene classes only.  Shared by the CPU test that holds the conditions of these inputs on the restatement alone and
the stepper's host hook to the restatement (test_camera_seams_cpu.py: a class that never reaches its seam fails there) and by the GPU test
that holds both kernels to the restatement on them (test_gpu_camera_seams.py).

Every coordinate of the two scenes is a multiple of 1/16 below 64, so differences of a lattice body and a face are exact in binary32.  The
two scenes put the same features at the same places where they can: an inside corner of two walls at (4, 4), a ceiling whose underside is
y = 3 over x in [8, 12], z in [-4, 0], a floor whose top is y = 0 - so most cases run in both.

A CASE is (class, scene, shape, the ten words of the initial body, ticks = [(moves, dt_ms, run_update)], world).  An ULP FAN is a case five
times with one input moved -2 .. +2 ulps (a move's length where the seam is in the move, else a coordinate of the body).  SEAMS names, per class, the comparisons of the restatement's observer
(tests/volume_camera_restatement.py) that the class's cases must reach with both sides equal - or within the fan where a side is not a
binary32 value - and with both outcomes.

Some seams of the list are not reachable by any input and are left out on purpose (each is argued where its class is built): `residual`
next to 1e-6 (it is 0 or at least 0.009); two capsule rays with equal cand and DIFFERENT normals (behind a hit at t only t' <= t - 0.009
hits; the one tie is at the clamp cand == 0, against one wall, and in a voxel grid not even that); a DENORMAL `pen` (pen = radius - t with t >= tMin = 0.001
and t <= radius: both operands are at least 0.001, so their binary32 difference is 0 or at least an ulp of 0.001 - the class holds the
smallest positive pen instead, one ulp of the radius); and an exit at exactly search_r that WINS the search (an embedded body has four walls
within the embed probe, a sixteenth of search_r at most, so a hit at search_r never is the nearest: the case is there, the ray's hit and miss
both occur, the body does not depend on it)."""
import numpy as np

import volume_camera_restatement as vr
from yetanotherconsolegameengine_amd import abi, scenes as _scenes
from yetanotherconsolegameengine_amd.scene import AmbientLight, Box, Material, PointLight, Scene, VolumeGrid, vec3

F32, F64 = np.float32, np.float64
H, V, JUMP, SHIFT = vr.MOVE_HORIZONTAL, vr.MOVE_VERTICAL, vr.MOVE_JUMP, vr.MOVE_SHIFT
SCENES = ("boxes", "voxels")
CLASSES = ("move_cutoff", "capsule_block", "capsule_tie", "slide", "vertical", "embed", "exit_tie", "push", "fan", "ground_state", "failsafe_timer",
           "limits")
WORLDS = {"boxes": (16.0, 4.0, 1.0), "voxels": (8.0, 2.0, 1.0)}            # WorldHeight, WaterLevel, VoxelSize.Y

# in ycge_body_shape's order: eye_height, collision_radius, probe_radius, ground_clearance, jump_speed, gravity_accel
SHAPES = {
    "default": abi.BODY_SHAPE_DEFAULT,                        # 1.7, 0.65, 0.35, 0.10: not dyadic - its seams are reached by fans
    "low": (0.75, 0.5, 0.25, 0.125, 4.0, 8.0),                # eye + clearance = 0.875 <= 1: the corrective fan (tMax 2.1) reaches the floor from a hover of 0.5
    "unit": (0.875, 0.5, 0.25, 0.125, 4.0, 8.0),              # eye + clearance = 1: a body 1.5 above the floor has the floor at the corrective fan's tMax AND hovers exactly 0.5
    "wide": (2.0, 2.0, 0.5, 0.125, 4.0, 8.0),                 # radius 2: the embed probe is 0.5, the walls of a one-cell shaft exactly at its tMax
}
SHAPE_GLOBALS = ("EyeHeight", "CollisionRadius", "ProbeRadius", "GroundClearance", "JumpSpeed", "GravityAccel")


def rest_y(shape, ground=0.0):
    """binary32 of ground + EyeHeight + GroundClearance as Update computes it (:111)"""
    s = SHAPES[shape]
    return F32(F64(ground) + F64(F32(s[0])) + F64(F32(s[3])))


# ------------------------------------------------------------------------------------------------------------------------ scenes
BOXES = [
    ((-48, -1, -48), (48, 0, 48)),                                                  # floor, top y = 0
    ((4, 0, -8), (5, 4, 8)), ((-8, 0, 4), (5, 4, 5)),                               # two walls, faces x = 4 and z = 4: an inside corner at (4, 4)
    ((-6.5, 0, -0.125), (-6.125, 4, 0.125)), ((-5.875, 0, -0.125), (-5.5, 4, 0.125)),         # the 0.25 shaft around (-6, 0): -x, +x,
    ((-6.125, 0, 0.125), (-5.875, 4, 0.5)), ((-6.125, 0, -0.5), (-5.875, 4, -0.125)),         # +z, -z
    ((-6.5, 0, -3.125), (-6.125, 4, -2.875)), ((-6.125, 0, -2.875), (-5.875, 4, -2.5)), ((-6.125, 0, -3.5), (-5.875, 4, -3.125)),   # the same around (-6, -3), open to +x
    ((-6.5, 0, -6.125), (-6.125, 0.625, -5.875)), ((-5.875, 0, -6.125), (-5.5, 0.625, -5.875)),          # the same around (-6, -6), 0.625 high: torso deep,
    ((-6.125, 0, -5.875), (-5.875, 0.625, -5.5)), ((-6.125, 0, -6.5), (-5.875, 0.625, -6.125)),          # the eye above it
    ((-0.0625, 0, -6.0625), (0.0625, 4.875, -5.9375)),                              # the 0.125 post around (0, -6); its top 4 above a low body's eye
    ((1.9375, 0, -6.125), (2.0625, 4, -5.875)),                                     # a 0.125 x 0.25 post around (2, -6): x exits nearer than z exits
    ((1, 0, -3), (3, 0.25, -1)),                                                    # a low step
    ((8, 3, -4), (12, 3.5, 0)),                                                     # a ceiling slab, underside y = 3
    ((0, 0, 6), (0.0625, 4, 12)),                                                   # a free-standing thin wall
    ((-3.5, 0, -14), (-3, 4, -10)), ((-2.25, 0, -14), (-1.75, 4, -10)),             # a corridor 0.75 wide around x = -2.625: narrower than a body
    ((7.9375, 0.8125, -8.0625), (8.0625, 0.9375, -7.9375)),                         # a 0.125 cube around a low body's eye at (8, 0.875, -8)
    ((40, -9, 40), (44, -8, 44)), ((40, -9.0625, 50), (44, -8.0625, 54)),           # platforms beside the floor: tops at the auto fan's tMax and 1/16 beyond
]


def _material():
    return Material(vec3(0.7, 0.7, 0.7), 0.0, 0.0)


def _voxel_grids():
    """two grids of unit voxels that share the face x = 8.  A: 16 x 8 x 16 cells from (-8, -1, -8): cell (i, j, k) is x in [i - 8, i - 7],
    y in [j - 1, j], z in [k - 8, k - 7].  B: 4 x 8 x 16 from (8, -1, -8)"""
    S = _scenes.STONE
    a = np.zeros((16, 8, 16, 2), np.int32)
    a[:, 0, :, 0] = S                                          # floor, top y = 0
    a[12, 1:5, 0:13, 0] = S                                    # wall, face x = 4
    a[0:13, 1:5, 12, 0] = S                                    # wall, face z = 4: the inside corner at (4, 4)
    a[1:4, 1:6, 2:5, 0] = S; a[2, 1:6, 3, 0] = 0               # a one-cell shaft around (-5.5, -4.5), walls up to y = 5
    a[1:4, 1:6, 7:10, 0] = S; a[2, 1:6, 8, 0] = 0; a[3, 1:6, 8, 0] = 0      # the same around (-5.5, 0.5), open to +x
    a[8, 1:5, 2, 0] = S                                        # a one-cell pillar, x in [0, 1], z in [-6, -5]
    a[8, 1:5, 14:16, 0] = S                                    # a free-standing wall one cell thick, face x = 0 over z in [6, 8]
    a[9, 1, 5:7, 0] = S; a[10, 1:3, 5:7, 0] = S; a[11, 1:4, 5:7, 0] = S       # a staircase up +x: tops y = 1, 2, 3 over x in [1, 4], z in [-3, -1]
    b = np.zeros((4, 8, 16, 2), np.int32)
    b[:, 0, :, 0] = S                                          # floor
    b[:, 4, 4:8, 0] = S                                        # a cell roof, underside y = 3 over x in [8, 12], z in [-4, 0]
    b[2, 1:3, 12, 0] = S                                       # a block in B, x in [10, 11], z in [4, 5]
    unit = vec3(1, 1, 1)
    return [VolumeGrid(a, vec3(-8, -1, -8), unit, _scenes.VoxelMaterialLookup, False), VolumeGrid(b, vec3(8, -1, -8), unit, _scenes.VoxelMaterialLookup, False)]


_SCENE_CACHE = {}


def scene(name):
    """one of SCENES (built once): the Scene the oracle and the library are both given"""
    if name not in _SCENE_CACHE:
        s = Scene()
        s.Ambient = AmbientLight(vec3(1, 1, 1), 0.1)
        if name == "boxes":
            s.Lights.append(PointLight(vec3(0.0, 6.0, 0.0), vec3(1, 1, 1), 40.0))
            for lo, hi in BOXES:
                s.Objects.append(Box(vec3(*lo), vec3(*hi), _material(), 0.0, 0.0))
        elif name == "voxels":
            s.IsVolumeScene = True
            s.Objects = _voxel_grids()
        else:
            raise KeyError(name)
        _SCENE_CACHE[name] = s
    return _SCENE_CACHE[name]


# ------------------------------------------------------------------------------------------------------------------------ helpers
def ulps(x, k):
    """x moved k binary32 values up (k < 0: down)"""
    x = F32(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf))
    return F32(x)


def ulp_of(x):
    return F32(np.spacing(F32(abs(float(x)))))


def _move_for_tmax(target, horizontal):
    """the move length a for which the first micro-step's tMax is exactly `target`: AttemptMoveHorizontal asks
    (float)(sqrt((double)(a * a)) + 1e-3) (:224, :288), AttemptMoveVertical (float)(|a| + 1e-3) (:309); found among the neighbours of
    target - 0.001.  With tMax a lattice value, a wall at a lattice distance is exactly at it"""
    a0 = F32(F64(target) - F64(1e-3))
    for k in range(-8, 9):
        a = ulps(a0, k)
        step = np.sqrt(F64(a * a)) if horizontal else F64(a)
        if F32(step + F64(1e-3)) == F32(target):
            return a
    raise AssertionError(("no move length gives tMax", target))


STEP_H_EIGHTH = _move_for_tmax(0.125, True)           # (both below every shape's maxStep, 0.175 at the least: step == remaining)
STEP_V_EIGHTH = _move_for_tmax(0.125, False)


class Case:
    def __init__(self, cls, scene_name, shape, name, pos, ticks, vel=0.0, timer=0.0, repel=(0.0, 0.0, 0.0), auto_placed=True, grounded=False, world=None,
                 family=None):
        self.cls, self.scene, self.shape, self.name = cls, scene_name, shape, name
        self.pos = tuple(F32(v) for v in pos)
        self.vel, self.timer, self.repel = F32(vel), F32(timer), tuple(F32(v) for v in repel)
        self.auto_placed, self.grounded = bool(auto_placed), bool(grounded)
        self.ticks = [(list(m), float(dt), bool(u)) for m, dt, u in ticks]
        self.world = tuple(float(F32(v)) for v in (world or WORLDS[scene_name]))
        self.family = family or name                           # the cases of one fan share it

    def clock(self):
        """what the bodies of one batch must share: the world and every tick's (dt_ms, run_update)"""
        return (self.world, tuple((dt, u) for _, dt, u in self.ticks))

    def body(self):
        b = abi.CameraBody()
        b.pos[:] = [float(v) for v in self.pos]
        b.vertical_velocity, b.shift_hold_timer = float(self.vel), float(self.timer)
        b.repel_vel[:] = [float(v) for v in self.repel]
        b.auto_placed, b.is_grounded = int(self.auto_placed), int(self.grounded)
        return b

    def camera(self, hit, observer=None):
        """the restatement's camera in this case's initial state (its shape is the caller's business: under_shape)"""
        cam = vr.VolumeCamera(hit, self.pos, *self.world, auto_placed=self.auto_placed, observer=observer)
        cam.verticalVelocity, cam.shiftHoldTimer, cam.repelVel, cam.isGrounded = self.vel, self.timer, [F32(v) for v in self.repel], self.grounded
        return cam

    def __repr__(self):
        return f"{self.cls}/{self.scene}/{self.shape}/{self.name}"


class under_shape:
    """the restatement's six shape globals as binary32 of the shape's values for the length of a `with`"""

    def __init__(self, shape):
        self.values = [F32(v) for v in SHAPES[shape]]

    def __enter__(self):
        self.saved = [getattr(vr, g) for g in SHAPE_GLOBALS]
        for g, v in zip(SHAPE_GLOBALS, self.values):
            setattr(vr, g, v)

    def __exit__(self, *exc):
        for g, v in zip(SHAPE_GLOBALS, self.saved):
            setattr(vr, g, v)


def shape_struct(shape):
    return abi.BodyShape(*SHAPES[shape])


# ------------------------------------------------------------------------------------------------------------------------ the cases
QUIET = 16.0


def _build():
    out = []

    def add(cls, scene_names, shape, name, pos, moves=(), dt=QUIET, update=True, ticks=None, **kw):
        for sn in ((scene_names,) if isinstance(scene_names, str) else scene_names):
            out.append(Case(cls, sn, shape, name, pos, ticks if ticks is not None else [(moves, dt, update)], **kw))

    def fan(cls, scene_names, shape, name, pos, axis, ks=(-2, -1, 0, 1, 2), **kw):
        """the case with pos[axis] moved k ulps"""
        for k in ks:
            p = list(pos)
            p[axis] = ulps(p[axis], k)
            add(cls, scene_names, shape, f"{name}{k:+d}", p, **dict({"family": name}, **kw))

    both = SCENES
    # (x, z) = (-3, 1) is open floor in both scenes: nothing within 1.0, so nothing in reach of the low, unit and default bodies put there

    def at_rest(shape, x, z, ground=0.0):
        return (x, rest_y(shape, ground), z)

    # ---- move_cutoff: lengths at the binary32 neighbours of 1e-6 (`remaining <= 1e-6`, `Math.Abs(dy) <= 1e-6`); (a, b) whose binary32
    # a * a + b * b rounds to either side; and a move that leaves `remaining` next to 1e-6 after its first full step
    e6 = F32(1e-6)
    for k in (-2, -1, 0, 1, 2):
        a = float(ulps(e6, k))
        add("move_cutoff", both, "low", f"h{k:+d}", at_rest("low", -3.0, 1.0), [(H, 0, a, 0.0), (H, 0, 0.0, -a)], family="h")
        add("move_cutoff", both, "default", f"v{k:+d}", at_rest("default", -3.0, 1.0), [(V, 0, a, 0.0), (V, 0, -a, 0.0)], family="v")
    r2 = F32(F64(1e-6) / np.sqrt(F64(2.0)))
    for k in range(-2, 3):
        a = float(ulps(r2, k))
        add("move_cutoff", both, "default", f"ab{k:+d}", at_rest("default", -3.0, 1.0), [(H, 0, a, a), (H, 0, -a, float(ulps(r2, -k)))], family="ab")
    # (0.6, 0.8) * 1e-6 and neighbours: the exact sum of squares lies above 1e-12 and its binary32 rounding on the float below - the move is
    # ignored where `delta.X * delta.X + delta.Z * delta.Z` is a float sum (Vec3 is three floats, :221), taken by one in doubles.  (Only this
    # way round: 1e-12 lies in the lower half of its float interval.)  Four of the family round across, four agree either way
    a0, b0 = F32(0.6e-6), F32(0.8e-6)
    for k, j in ((0, 0), (-1, 1), (1, -1), (-3, 2), (-1, 0), (1, 0), (-4, 0), (4, 0)):
        a, b = ulps(a0, k), ulps(b0, j)
        add("move_cutoff", both, "low", f"round{k:+d}{j:+d}", at_rest("low", -3.0, 1.0), [(H, 0, float(a), float(b)), (H, 0, float(-b), float(a))], family="round")
    for shape, max_step in (("low", 0.175), ("default", 0.2275)):
        for k in range(-2, 3):
            a = float(F32(F32(max_step + 1e-6) + F32(k) * ulp_of(max_step)))
            add("move_cutoff", both, shape, f"tail{k:+d}", at_rest(shape, -3.0, 1.0), [(H, 0, a, 0.0)], family="tail-" + shape)

    # ---- capsule_block: the wall x = 4 straight ahead.  cand = t - 0.01 around 1e-5: the body at fl(4 - 0.01001), moved in ulps of 4;
    # the wall exactly at the first micro-step's tMax = 0.125 (step == remaining), the body on the lattice and one ulp either side
    for shape in ("low", "default"):
        y = rest_y(shape)
        fan("capsule_block", both, shape, "cand", (F32(4.0) - F32(0.01001), y, 0.0), 0, moves=[(H, 0, 0.05, 0.0)])
        fan("capsule_block", both, shape, "tmax", (3.875, y, 0.0), 0, moves=[(H, 0, float(STEP_H_EIGHTH), 0.0)])
        fan("capsule_block", both, shape, "tmax-z", (0.0, y, 3.875), 2, moves=[(H, 0, 0.0, float(STEP_H_EIGHTH))])
    add("capsule_block", both, "low", "second-step", (3.7, rest_y("low"), -2.0), [(H, 0, 0.5, 0.0)])

    # ---- capsule_tie: `cand < best` with both sides equal.  LimitStepByRay asks every ray with tMax = best + 1e-3 and takes cand = t - 0.01,
    # so behind a hit at t only a ray with t' <= t - 0.009 hits at all: two capsule rays of one t never both reach the comparison - straight
    # at a wall the first of six equal rays hits, five miss; into the inside corner at (4, 4) along dx == dz, where the side rays meet
    # different walls at one t and the centre ray the shared edge, the same (these cases are kept: the tie is then inside Scene.Hit).  The
    # one reachable tie is at the clamp cand = Math.Max(0, t - 0.01) = 0: a wall whose face is x = 0 exactly tMin = 0.001f ahead (the body
    # at x = -0.001f, exact) - the first ray makes best 0, tMax becomes (float)(0 + 1e-3) == tMin, and every later ray of the six hits at
    # t == tMin == tMax with cand == best == 0.  One ulp nearer the rays start below tMin, one ulp farther they end beyond tMax.
    # In a voxel grid not even that: VolumeGrid.Hit takes its first sample at tMin + 1e-6 (VolumeGrid.cs:99-231), so a solid cell that near
    # is reported at 0.001001 > tMax; the voxel cases stay for that path, SEAMS asks the tie of the boxes alone
    for shape in ("low", "default"):
        fan("capsule_tie", both, shape, "clamp", (-F32(0.001), rest_y(shape), 7.0), 0, moves=[(H, 0, 0.05, 0.0)])
        fan("capsule_tie", both, shape, "clamp-far", (-F32(0.0109), rest_y(shape), 7.0), 0, moves=[(H, 0, 0.05, 0.0)], ks=(-1, 0, 1))
    for shape in ("low", "default", "wide"):
        y = rest_y(shape)
        for p, m in ((3.0, 0.5), (2.5, 2.0)):
            add("capsule_tie", both, shape, f"corner{p}", (p, y, p), [(H, 0, m, m)], family="corner")
        fan("capsule_tie", both, shape, "offdiag", (2.0, y, 2.0), 0, moves=[(H, 0, 1.0, 1.0)], ks=(-1, 1))
        add("capsule_tie", both, shape, "straight", (2.0, y, -2.0), [(H, 0, 2.0, 0.0)], family="straight")

    # ---- slide: headings whose slide vector is about 1e-6f long; a heading exactly perpendicular to the wall (length 0, both zero signs).
    # `residual > 1e-6` has no seam: residual = step - best is 0 without a hit, and a hit has t <= tMax = step + 1e-3 and best = t - 0.01,
    # so residual >= 0.009 less a rounding (the least is the wall exactly at tMax: capsule_block's cases); where the clamp makes best 0
    # the micro-step is blocked before the comparison.  The class holds both sides, never the cut-off
    for shape in ("low", "default"):
        y = rest_y(shape)
        for k in range(-2, 3):
            e = float(F32(0.125) * ulps(e6, k))
            add("slide", both, shape, f"length{k:+d}", (3.95, y, 0.0), [(H, 0, 0.125, e)], family="length")
        add("slide", both, shape, "perpendicular", (3.95, y, 0.0), [(H, 0, 0.125, 0.0)], family="perpendicular")
        add("slide", both, shape, "perpendicular-0", (3.95, y, 0.0), [(H, 0, 0.125, -0.0)], family="perpendicular")
        add("slide", both, shape, "oblique", (3.5, y, 0.0), [(H, 0, 1.0, 0.5)], family="oblique")

    # ---- vertical: the ceiling's underside y = 3 and the floor's top y = 0 at cand around 1e-5 and exactly at tMax = 0.125
    for shape in ("low", "default"):
        fan("vertical", both, shape, "ceiling-cand", (10.0, F32(3.0) - F32(0.01001), -2.0), 1, moves=[(V, 0, 0.05, 0.0)], timer=0.15)
        fan("vertical", both, shape, "floor-cand", (-3.0, F32(0.01001), 1.0), 1, moves=[(V, 0, -0.05, 0.0)], timer=0.15)
        fan("vertical", both, shape, "ceiling-tmax", (10.0, 2.875, -2.0), 1, moves=[(V, 0, float(STEP_V_EIGHTH), 0.0)], timer=0.15)
        fan("vertical", both, shape, "floor-tmax", (-3.0, 0.125, 1.0), 1, moves=[(V, 0, -float(STEP_V_EIGHTH), 0.0)], timer=0.15)
    add("vertical", both, "default", "rise-2", (10.0, 1.8, -2.0), [(V, 0, 2.0, 0.0)], timer=0.15)

    # ---- embed: walls at t == probe on all four sides (low in the 0.25 shaft of boxes: probe 0.125; wide in the one-cell shaft of voxels:
    # probe 0.5), one ulp off either way; three sides only; the eye above the walls and the torso between them (the `k == 3` short cut of
    # cam_commit is NOT taken, all eight rays are asked); a body inside a solid voxel on a cell's face, edge and corner (tMin = 0)
    for axis in (0, 2):
        fan("embed", "boxes", "low", f"shaft-{'xz'[axis // 2]}", (-6.0, rest_y("low"), 0.0), axis)
        fan("embed", "voxels", "wide", f"shaft-{'xz'[axis // 2]}", (-5.5, rest_y("wide"), -4.5), axis)
    fan("embed", "boxes", "default", "shaft", (F32(-5.875) - F32(0.1625), rest_y("default"), 0.0), 0)
    fan("embed", "voxels", "default", "shaft", (F32(-5.0) - F32(0.1625), rest_y("default"), -4.5), 0)
    add("embed", "boxes", "low", "three-sides", (-6.0, rest_y("low"), -3.0))
    add("embed", "voxels", "wide", "three-sides", (-5.5, rest_y("wide"), 0.5))
    add("embed", "boxes", "low", "torso-only", (-6.0, rest_y("low"), -6.0))            # eye 0.875 above the 0.625 walls, torso 0.5 between them
    add("embed", "voxels", "wide", "torso-only", (-5.5, 5.5, -4.5))                    # eye 5.5 above the walls (y = 5), torso 4.5 between them
    for name, p in (("solid-centre", (-6.5, 2.5, -4.5)), ("solid-face", (-6.0, 2.5, -4.5)), ("solid-face-y", (-6.5, 3.0, -4.5)), ("solid-edge", (-6.0, 2.5, -5.0)),
                    ("solid-corner", (-6.0, 3.0, -5.0)), ("outer-face", (-7.0, 2.5, -4.5)), ("shared-face", (8.0, 0.0, 2.0)), ("floor-corner", (8.0, 0.0, 8.0))):
        for shape in ("default", "wide"):
            add("embed", "voxels", shape, name, p, family="solid")

    # ---- exit_tie: equal exit distances in four directions (the centre of the 0.125 post), in two (the 0.125 x 0.25 post), in six (the
    # 0.125 cube around the eye), eye and torso rays tying throughout: the first direction asked (+x) wins; the post's top exactly at
    # search_r = 4 above the eye.  A body inside a solid voxel is answered at tMin + 1e-6 by all twelve rays - a twelve-way tie.  In the voxel
    # scene no exit lies at search_r: an embedded body there is inside a solid cell (every ray at 1e-6) or wide in the one-cell shaft, eye
    # and torso on half-integers with the faces on integers and search_r = 8 an integer; SEAMS asks that of the boxes alone
    add("exit_tie", "boxes", "low", "four", (0.0, rest_y("low"), -6.0), family="four")
    add("exit_tie", "boxes", "default", "four", (0.0, rest_y("default"), -6.0), family="four")
    add("exit_tie", "boxes", "low", "two", (2.0, rest_y("low"), -6.0), family="two")
    add("exit_tie", "boxes", "default", "two", (2.0, rest_y("default"), -6.0), family="two")
    add("exit_tie", "boxes", "low", "six", (8.0, 0.875, -8.0), family="six")
    fan("exit_tie", "boxes", "low", "search-r", (0.0, 0.875, -6.0), 1)
    add("exit_tie", "voxels", "default", "four", (0.5, 2.5, -5.5), family="four")                # the pillar's cell: +-x, +-z at 0.5
    add("exit_tie", "voxels", "wide", "four", (0.5, 2.5, -5.5), family="four")
    add("exit_tie", "voxels", "default", "two", (0.25, 2.5, -5.5), family="two")
    add("exit_tie", "voxels", "default", "six", (0.5, 0.5, -5.5), family="six")                  # eye in the pillar's lowest cell, torso in the floor's
    add("exit_tie", "voxels", "wide", "two", (4.5, 2.5, 0.0), family="two")                      # inside the wall x in [4, 5], on a cell face in z

    # ---- push: the wall x = 4 at exactly the radius (pen == 0) and one ulp either side (the smallest positive pen); a diagonal ray into a
    # wall's end edge; a body in a corridor narrower than itself, where ray after ray moves it (the most dropped windows)
    for shape in ("low", "wide"):
        r = SHAPES[shape][1]
        fan("push", both, shape, "radius", (4.0 - r, rest_y(shape), 0.0), 0, dt=0.0)
        fan("push", both, shape, "radius-z", (0.0, rest_y(shape), 4.0 - r), 2, dt=0.0)
    fan("push", both, "default", "radius", (F32(4.0) - F32(0.65), rest_y("default"), 0.0), 0, dt=0.0)
    add("push", both, "low", "edge", (3.75, rest_y("low"), -8.25), dt=0.0)
    add("push", both, "default", "edge", (3.75, rest_y("default"), -8.25), dt=0.0)
    add("push", "boxes", "low", "wedged", (-2.625, rest_y("low"), -12.0), dt=0.0)
    add("push", "boxes", "default", "wedged", (-2.625, rest_y("default"), -12.0), dt=0.0)
    add("push", "voxels", "wide", "wedged", (-5.5, rest_y("wide"), -4.5), dt=0.0)             # (the one-cell shaft: embedded first, then wedged)
    add("push", "voxels", "default", "wedged", (-5.5, rest_y("default"), -4.5), dt=0.0)
    add("push", "boxes", "low", "thin-wall-left", (-0.25, rest_y("low"), 9.0), dt=0.0)
    add("push", "boxes", "low", "thin-wall-right", (0.3125, rest_y("low"), 9.0), dt=0.0)

    # ---- fan: a probe ray exactly down a side face of the low step (boxes) and down a cell's edge of the staircase (voxels): body x = 1 -
    # probe_radius; floor_candidate around pos.y + 0.05f; probe rays with equal y (any level floor); ground exactly at tMax of the ground
    # fan (3.6 from pos.y + 0.6f: a body at y = 3), the corrective fan (2.1: y = 1.5) and the auto placement; auto placement with
    # WorldHeight + 16 == 4096 and above it, and with nothing under the body
    for shape in ("low", "unit"):
        pr = SHAPES[shape][2]
        fan("fan", "boxes", shape, "side-face", (1.0 - pr, rest_y(shape), -2.0), 0, dt=0.0)
        fan("fan", "voxels", shape, "cell-edge", (1.0 - pr, rest_y(shape), -3.0), 0, dt=0.0)
        fan("fan", "voxels", shape, "cell-face", (1.0 - pr, rest_y(shape), -2.0), 0, dt=0.0)
        fan("fan", "boxes", shape, "guard", (1.5, F32(rest_y(shape, 0.25)) - F32(0.05), -2.0), 1, dt=0.0)
        fan("fan", "voxels", shape, "guard", (1.5, F32(rest_y(shape, 1.0)) - F32(0.05), -2.0), 1, dt=0.0)
        fan("fan", both, shape, "ground-tmax", (-3.0, 3.0, 1.0), 1, dt=0.0)
        fan("fan", both, shape, "corr-tmax", (-3.0, 1.5, 1.0), 1, dt=0.0)
        add("fan", "boxes", shape, "best-rises", (1.0 - pr / 2, rest_y(shape, 0.25), -2.0), dt=0.0, family="best")      # centre ray on the floor, the +x ray on the step
        add("fan", "voxels", shape, "best-rises", (1.0 - pr / 2, rest_y(shape, 1.0), -2.0), dt=0.0, family="best")
        add("fan", both, shape, "best-level", (-3.0, rest_y(shape), 1.0), dt=0.0, family="best")
    fan("fan", both, "default", "ground-tmax", (-3.0, 3.0, 1.0), 1, dt=0.0)
    fan("fan", "boxes", "default", "guard", (1.5, F32(rest_y("default", 0.25)) - F32(0.05), -2.0), 1, dt=0.0)
    for shape in ("default", "low"):
        add("fan", "boxes", shape, "auto-tmax", (42.0, 5.0, 42.0), auto_placed=False, family="auto")
        add("fan", "boxes", shape, "auto-beyond", (42.0, 5.0, 52.0), auto_placed=False, family="auto")
    for shape in ("default",):
        add("fan", both, shape, "auto-nothing", (56.0, 5.0, 56.0), auto_placed=False, family="auto")
        add("fan", both, shape, "auto", (-3.0, 9.0, 1.0), auto_placed=False, family="auto")
        add("fan", both, shape, "auto-embedded", (4.5, 2.0, 0.0), auto_placed=False, family="auto")
        for name, wh in (("auto-4096", 4080.0), ("auto-4096-1", ulps(4080.0, -1)), ("auto-above", 4096.0), ("auto-4096+1", ulps(4080.0, 1))):
            add("fan", both, shape, name, (-3.0, 9.0, 1.0), auto_placed=False, world=(wh, 4.0, 1.0), family="auto-4096")

    # ---- ground_state: new_y == floor_y (a body at rest, dt 0) and one ulp either side; pos.y - floor_y around 0.05; pos.y - f2 around 0.5
    # (dyadic shapes: exactly 0.5); dt of 0, negative and 100 ms; a jump in the tick after is_grounded was decided at its threshold
    for shape in ("low", "unit", "default"):
        y = rest_y(shape)
        fan("ground_state", both, shape, "rest", (-3.0, y, 1.0), 1, dt=0.0)
        for dt in (-0.0, -5.0, 100.0):
            add("ground_state", both, shape, f"rest-dt{dt:g}", (-3.0, y, 1.0), dt=dt, vel=-0.5, family="rest")
        fan("ground_state", both, shape, "guard", (-3.0, F32(y + F32(0.05)), 1.0), 1, dt=0.0,
            ticks=[([], 0.0, True), ([(JUMP, 0, 0.0, 0.0)], QUIET, True), ([], QUIET, True)])
        fan("ground_state", both, shape, "hover", (-3.0, F32(y + F32(0.5)), 1.0), 1, dt=0.0)
        add("ground_state", both, shape, "falling", (-3.0, F32(y + F32(0.3)), 1.0), vel=-2.0, dt=100.0)
        add("ground_state", both, shape, "rising", (-3.0, y, 1.0), vel=3.0, dt=100.0, grounded=True)
    add("ground_state", both, "default", "on-the-step", (2.0, rest_y("default", 0.25), -2.0), dt=0.0)

    # ---- failsafe_timer: y around -10 with the fly timer running (no gravity); the timer minus dt around 0 (0.15 s against 150 ms, dt in
    # ulps; the tick after shows whether gravity acted); MOVE_SHIFT then MOVE_JUMP in one tick
    for shape in ("default", "low"):
        fan("failsafe_timer", both, shape, "minus-ten", (-3.0, -10.0, 1.0), 1, timer=1.0, vel=-1.0, repel=(0.5, -0.25, 2.0))
        for k in range(-2, 3):
            dt = float(ulps(150.0, k))
            add("failsafe_timer", both, shape, f"timer{k:+d}", (-3.0, 3.0, 1.0), timer=0.15, ticks=[([], dt, True), ([], QUIET, True)], family="timer")
        add("failsafe_timer", both, shape, "timer-early", (-3.0, 3.0, 1.0), timer=0.15, ticks=[([], 149.99, True), ([], QUIET, True)], family="timer")
        add("failsafe_timer", both, shape, "timer-late", (-3.0, 3.0, 1.0), timer=0.15, ticks=[([], 150.01, True), ([], QUIET, True)], family="timer")
        add("failsafe_timer", both, shape, "shift-jump", (-3.0, rest_y(shape), 1.0), grounded=True,
            ticks=[([(SHIFT, 0, 0.0, 0.0), (JUMP, 0, 0.0, 0.0)], QUIET, True), ([], QUIET, True)], family="shift-jump")
        add("failsafe_timer", both, shape, "jump-shift", (-3.0, rest_y(shape), 1.0), grounded=True,
            ticks=[([(JUMP, 1, 0.0, 0.0), (JUMP, 0, 0.0, 0.0), (SHIFT, 0, 0.0, 0.0)], QUIET, True), ([], QUIET, True)], family="shift-jump")
        add("failsafe_timer", both, shape, "air-jump", (-3.0, F32(rest_y(shape) + F32(1.0)), 1.0),
            ticks=[([(JUMP, 0, 0.0, 0.0)], QUIET, True), ([], QUIET, True)], family="shift-jump")
        add("failsafe_timer", both, shape, "falls-out", (60.0, -9.99, 60.0), vel=-3.0, dt=100.0, family="falls")

    # ---- limits: 32 moves in one tick; a move of length exactly 64 (wide: 92 micro-steps); bodies at |x| or |z| = 2^24 and 2^30 - the scene
    # is far away, every ray misses, the steps are absorbed by rounding and the arithmetic must still agree
    for shape in ("default", "low"):
        y = rest_y(shape)
        add("limits", both, shape, "32-moves", (-3.0, y, 1.0), [(H, 0, 0.01 * (1 + i % 3), 0.01 * (i % 2)) for i in range(32)])
        add("limits", both, shape, "32-mixed", (3.5, y, 3.5), [((H, 0, 0.03, 0.02), (V, 0, 0.02, 0.0), (JUMP, 0, 0.0, 0.0), (H, 0, -0.01, 0.04))[i % 4] for i in range(32)])
        for e, big in (("2^24", 2.0 ** 24), ("2^30", 2.0 ** 30)):
            add("limits", both, shape, f"x{e}", (big, y, 0.0), [(H, 0, 0.5, 0.0), (V, 0, 0.5, 0.0)])
            add("limits", both, shape, f"-x{e}", (-big, y, 7.0), [(H, 0, 0.5, 0.3)])
            add("limits", both, shape, f"z{e}", (7.0, y, big), [(H, 0, 0.5, 0.3), (H, 0, -0.4, -0.4)])
            add("limits", both, shape, f"-z{e}", (0.0, y, -big), [(H, 0, 0.0, -0.5)], timer=0.15)
    add("limits", both, "wide", "length-64", (-40.0, 9.0, 20.0), [(SHIFT, 0, 0.0, 0.0), (H, 0, 64.0, 0.0)])
    add("limits", both, "wide", "length-64-down", (20.0, 50.0, 20.0), [(SHIFT, 0, 0.0, 0.0), (V, 0, -64.0, 0.0)])
    return out


CASES = _build()


def cases(scene_name=None, cls=None, shape=None):
    return [c for c in CASES if (scene_name is None or c.scene == scene_name) and (cls is None or c.cls == cls) and (shape is None or c.shape == shape)]


def batches(scene_name):
    """the cases of a scene grouped into the batches ycge_volume_bodies_tick can take: one world, one (dt_ms, run_update) a tick"""
    groups = {}
    for c in cases(scene_name):
        groups.setdefault(c.clock(), []).append(c)
    return list(groups.values())


# ------------------------------------------------------------------------------------------------------------------------ the restatement
def restate(case, hit, log=None):
    """the restatement over one case: ([(body words, counters)] after every tick, the most micro-steps one move took).  log: a list that
    takes the observer's (name, left, right, outcome) tuples"""
    import volume_camera_cases as vc
    with under_shape(case.shape):
        cam = case.camera(hit, None if log is None else (lambda *rec: log.append(rec)))
        rows = []
        for moves, dt_ms, run_update in case.ticks:
            counters = cam.tick(moves, dt_ms, run_update)
            rows.append((vc.restatement_words(cam), counters))
    return rows, cam.max_micro


# ------------------------------------------------------------------------------------------------------------------------ the seams
# class -> [(comparison of the observer, how near its two sides must come, which scenes)].  0: both sides bit-equal somewhere.  A positive
# number: a side is no binary32 value (1e-6, 1e-5 and 0.05 as doubles) or the compared distance moves in ulps of a coordinate near 4 - three
# steps of the fan that reaches it, written out.  None: a comparison of two booleans, both outcomes are all that is asked.
# For every seam the class's cases must come that near in the scene, and the cases of the fans (families) that do must show both outcomes;
# for a "hit:" seam - rec.T against the ray's tMax - the outcome is the hit itself: the cases of such a fan differ in how many of those
# rays hit.
U4, U1, UE6 = 2.0 ** -22, 2.0 ** -24, 2.0 ** -43        # an ulp below 4, below 1 and of 1e-6
SEAMS = {
    "move_cutoff": [("h_cutoff", 3 * UE6, SCENES), ("v_cutoff", 3 * UE6, SCENES), ("h_remaining", 3 * 2.0 ** -26, SCENES)],      # (the tail: ulps of 0.2)
    "capsule_block": [("caps_blocked", 3 * U4, SCENES), ("hit:caps", 0, SCENES)],
    "capsule_tie": [("caps_cand", 0, ("boxes",)), ("hit:caps", 0, ("boxes",))],            # (voxels: see the class)
    "slide": [("slide_length", 3 * UE6, SCENES), ("residual", None, SCENES)],
    "vertical": [("vert_blocked", 3 * U4, SCENES), ("hit:vert", 0, SCENES)],
    "embed": [("hit:embed", 0, SCENES), ("embedded_torso", None, SCENES)],
    "exit_tie": [("exit_t", 0, SCENES), ("hit:exit", 0, ("boxes",))],                      # (voxels: see the class)
    "push": [("pen", 0, SCENES), ("hit:push", 0, SCENES)],
    "fan": [("hit:fan", 0, SCENES), ("fan_accept", 3 * U1 * 2, SCENES), ("fan_best", 0, SCENES), ("probe_top", 0, SCENES), ("auto_ground", None, SCENES)],
    "ground_state": [("snap", 0, SCENES), ("grounded", 3 * U1 * 2, SCENES), ("hover", 0, SCENES), ("dt_negative", 0, SCENES), ("jump_grounded", None, SCENES)],
    "failsafe_timer": [("fail_safe", 0, SCENES), ("timer_left", 3 * 2.0 ** -16 * 1e-3, SCENES), ("jump_grounded", None, SCENES)],      # (ulps of 150 ms, in seconds)
    "limits": [],
}


def seam_report(entries, name, tol):
    """entries: [(case, observer log)] of one class and scene.  (cases that come within tol, cases that reach it exactly, the outcomes of
    the comparison among the fans that come within tol, whether some such fan's cases differ in their count of true outcomes)"""
    near, exact, fams = set(), set(), set()
    for case, log in entries:
        for n, left, right, outcome in log:
            if n != name: continue
            if tol is None:
                near.add(case); exact.add(case); fams.add(case.family)
            elif left is not None and right is not None:
                d = abs(float(left) - float(right))
                if d <= tol: near.add(case); fams.add(case.family)
                if d == 0.0: exact.add(case)
    outcomes, counts = set(), {}
    for case, log in entries:
        if case.family in fams:
            mine = [bool(o) for n, _, _, o in log if n == name]
            outcomes |= set(mine)
            counts.setdefault(case.family, set()).add(sum(mine))
    return near, exact, outcomes, any(len(v) > 1 for v in counts.values())


# ------------------------------------------------------------------------------------------------------------------------ a child process
def _run_cases_on_the_device():
    """every default-shape case through ycge_volume_camera_tick in THIS process (tests/test_gpu_camera_seams.py starts it with
    YCGE_CAMERA_HOST=1): one JSON line {scene: [[[body words, info] per tick] per case]}"""
    import json
    import volume_camera_cases as vc
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import flatten
    out = {}
    for name in SCENES:
        g = RaytraceRenderer(flatten(scene(name)), 32, 16, 45.0, 1)
        out[name] = []
        for c in cases(name, shape="default"):
            b, w = c.body(), abi.CameraWorld(*c.world)
            rows = []
            for moves, dt_ms, run_update in c.ticks:
                info = g.CameraTick(b, w, moves, dt_ms, run_update)
                rows.append([[int(v) for v in vc.body_words(b)], info])
            out[name].append(rows)
        g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    import sys
    if "--run-cases" in sys.argv:
        _run_cases_on_the_device()
