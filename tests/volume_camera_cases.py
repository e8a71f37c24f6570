"""What tests/test_volume_camera_cpu.py and tests/test_gpu_volume_camera.py share: the two scenes, the drawn sequences of ticks and moves,
the oracle's Scene.Hit as the restatement's callable and as the hook's C callback, and the comparison of a body with the restatement's.

The sequences are drawn here, on the CPU; SEEDS were chosen by running the restatement alone (test_sequences_reach_every_event asserts
what they were chosen for: every event counter non-zero somewhere, no move near the micro-step cap)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import volume_camera_restatement as vr
from yetanotherconsolegameengine_amd import abi, scenes
from yetanotherconsolegameengine_amd.scene import AmbientLight, Box, Material, PointLight, Scene, flatten, vec3

F32 = np.float32
EVENTS = ("micro_steps", "blocked_steps", "slides", "push_outs", "embedded_resolutions", "ground_snaps", "auto_placements", "fail_safes")
WORLD5 = (128.0, 32.0, 1.0)          # the reduced config-5 world: WorldHeight 128, WaterLevel max(1, 128 / 4), VoxelSize.Y 1
WORLD_BOXES = (16.0, 4.0, 1.0)


# ------------------------------------------------------------------------------------------------------------------------ scenes
def box_scene(extra=()):
    """analytic boxes, no grid: a floor slab (top y = 0), four walls of an 8 x 8 room, a pillar, a low step, a block and a thin post
    to start inside of"""
    m = Material(vec3(0.7, 0.7, 0.7), 0.0, 0.0)
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.1)
    s.Lights.append(PointLight(vec3(0.0, 6.0, 0.0), vec3(1, 1, 1), 40.0))
    boxes = [((-6, -1, -6), (6, 0, 6)),                                                      # floor
             ((-6, 0, -5), (-4, 4, 5)), ((4, 0, -5), (6, 4, 5)), ((-6, 0, -6), (6, 4, -4)), ((-6, 0, 4), (6, 4, 6)),     # walls: the room is |x|, |z| < 4
             ((1.0, 0, 1.0), (2.0, 3, 2.0)),                                                  # pillar
             ((-3.0, 0, -3.0), (-1.5, 0.4, -1.5)),                                            # low step
             ((-3.5, 0, 1.5), (-1.0, 3, 3.5)),                                                # block
             ((2.9, 0, -3.2), (3.1, 3, -3.0))]                                                # a post thinner than the embed probe: start 1 is inside it
    for lo, hi in list(boxes) + list(extra):
        s.Objects.append(Box(vec3(*lo), vec3(*hi), m, 0.0, 0.0))
    return s


def voxel_scene():
    """the reduced config-5 voxel world the query tests use (frame_pair(oracle, 5, (160, 45, 1))'s scene)"""
    sc, _, _, _, pose = scenes.config_scene(5, small=True, t01=0.25)
    return sc, pose


SCENES = ("voxels", "boxes")


def make_scene(name):
    """(scene, world triple, start positions the sequences draw from)"""
    if name == "voxels":
        sc, pose = voxel_scene()
        x, y, z = pose["pos"]
        starts = [(x, y, z), (x + 7.3, y + 6.0, z - 4.1), (x - 11.6, y + 3.0, z + 9.7), (x + 3.2, y - 6.5, z + 2.4), (x - 20.3, y + 1.0, z - 17.2),
                  (x + 1.5, -15.0, z + 1.5)]                       # (the fourth is under ground, the last below the fail-safe)
        return sc, WORLD5, starts
    starts = [(0.0, 1.8, 0.0), (3.0, 1.8, -3.1), (-2.2, 1.2, 2.4), (1.5, 2.0, 1.4), (-2.3, 2.4, -2.2), (0.3, 5.0, 0.2), (0.5, -12.0, 0.5)]
    return box_scene(), WORLD_BOXES, starts


# ------------------------------------------------------------------------------------------------------------------------ Scene.Hit
def oracle_hit(o):
    """the restatement's callable over an OracleRenderer's orc_scene_hit ({hit, object, sub, t, P, N, albedo})"""
    def hit(origin, d, tmin, tmax):
        rec = o.scene_hit([float(v) for v in origin], [float(v) for v in d], float(tmin), float(tmax))
        if rec[0] == 0:
            return None
        return F32(rec[3]), (F32(rec[7]), F32(rec[8]), F32(rec[9]))
    return hit


def c_callback(hit):
    """a Python hit(o, d, tmin, tmax) as the hook's int hit(void *user, const float ray[8], float rec[7]); counts its calls in .calls"""
    def cb(_user, ray, rec):
        cb.calls += 1
        r = hit([F32(ray[0]), F32(ray[1]), F32(ray[2])], [F32(ray[3]), F32(ray[4]), F32(ray[5])], F32(ray[6]), F32(ray[7]))
        if r is None:
            return 0
        rec[0] = float(r[0])
        rec[4], rec[5], rec[6] = float(r[1][0]), float(r[1][1]), float(r[1][2])
        return 1
    cb.calls = 0
    fn = abi.CAMERA_HIT_FN(cb)
    fn.py = cb
    return fn


def bind_hook(lib):
    for name, (res, args) in abi.CAMERA_HOOK_PROTOTYPES.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def tick_hook(lib, body, world, moves, dt_ms, run_update, cb, windowed):
    """ycge_test_camera_tick_host: (rc, info dict, message)"""
    recs = (abi.CameraMove * max(1, len(moves)))(*[abi.CameraMove(int(k), int(s), float(a), float(b)) for k, s, a, b in moves])
    info = abi.CameraTickInfo()
    msg = C.create_string_buffer(256)
    rc = lib.ycge_test_camera_tick_host(C.byref(body), C.byref(world), recs if moves else None, len(moves), float(dt_ms), 1 if run_update else 0,
                                        C.byref(info), cb, None, 1 if windowed else 0, msg, 256)
    return rc, {n: int(getattr(info, n)) for n, _ in abi.CameraTickInfo._fields_}, msg.value.decode()


# ------------------------------------------------------------------------------------------------------------------------ bodies
def new_body(pos, auto_placed):
    b = abi.CameraBody()
    b.pos[:] = [float(F32(v)) for v in pos]
    b.auto_placed = 1 if auto_placed else 0
    return b


def body_words(b):
    """the 40 bytes of a ycge_camera_body as ten uint32"""
    return np.frombuffer(bytes(b), np.uint32).copy()


def restatement_words(cam):
    f, (ap, gr) = cam.body()
    return np.concatenate([f.view(np.uint32), np.array([ap, gr], np.uint32)])


def assert_same(b, info, want_words, counters, what):
    """a library body and info against the restatement's after the same tick, bit for bit"""
    got = body_words(b)
    assert np.array_equal(got, want_words), (what, "body", got.view(F32)[:8], want_words.view(F32)[:8], got[8:], want_words[8:])
    for k in ("rays_committed",) + EVENTS:
        assert info[k] == counters[k], (what, k, info[k], counters[k])


# ------------------------------------------------------------------------------------------------------------------------ sequences
def draw_sequence(seed, starts, n_ticks=10):
    """(start, auto_placed, [(moves, dt_ms, run_update)]): walks, shift-flight, jumps, vertical strafes, dt from 0 to 100 ms"""
    rng = np.random.default_rng(seed)
    start = starts[seed % len(starts)]
    auto_placed = bool(seed % 4 != 3)                     # (every fourth sequence starts with the auto placement)
    yaw = F32(rng.uniform(-np.pi, np.pi))
    ticks = [([], 16.0, True)]                            # a quiet first tick: a start inside geometry is resolved before anything moves it
    for _ in range(n_ticks - 1):
        dt_ms = F32(rng.choice([0.0, 4.0, 16.0, 33.0, 100.0]) if rng.random() < 0.7 else rng.uniform(0.0, 100.0))
        dt = dt_ms * F32(0.001)
        moves = []
        for _ in range(int(rng.integers(0, 4))):
            kind = rng.choice(["walk", "walk", "strafe", "fly", "rise", "jump", "turn"])
            shift = bool(rng.random() < 0.3)
            if kind == "turn":
                yaw = F32(yaw + F32(rng.uniform(-1.5, 1.5)))
                continue
            speed = F32(6.0) * (F32(30.0) if shift or kind == "fly" else F32(1.0))
            if shift or kind == "fly":
                moves.append((vr.MOVE_SHIFT, 0, 0.0, 0.0))
            k = speed * max(dt, F32(0.004))
            sy, cy = F32(np.sin(yaw)), F32(np.cos(yaw))
            sign = F32(rng.choice([-1.0, 1.0]))
            if kind in ("walk", "fly"):
                moves.append((vr.MOVE_HORIZONTAL, 0, float((sign * sy) * k), float((sign * -cy) * k)))
            elif kind == "strafe":
                moves.append((vr.MOVE_HORIZONTAL, 0, float((sign * cy) * k), float((sign * sy) * k)))
            elif kind == "rise":
                moves.append((vr.MOVE_VERTICAL, 0, float(sign * k), 0.0))
            else:
                moves.append((vr.MOVE_JUMP, 1 if shift else 0, 0.0, 0.0))
        ticks.append((moves, float(dt_ms), bool(rng.random() < 0.9)))
    return start, auto_placed, ticks


SEEDS = {"voxels": (0, 3, 5, 6, 7, 9, 11), "boxes": (0, 1, 2, 3, 6, 7, 8, 10)}


def run_restatement(hit, world, seq):
    """the restatement over one sequence: [(body words, counters)] after every tick, and the camera"""
    start, auto_placed, ticks = seq
    cam = vr.VolumeCamera(hit, start, *world, auto_placed=auto_placed)
    out = []
    for moves, dt_ms, run_update in ticks:
        counters = cam.tick(moves, dt_ms, run_update)
        out.append((restatement_words(cam), counters))
    return out, cam


# ------------------------------------------------------------------------------------------------------------------------ a child process
def _run_sequences_on_the_device():
    """every committed sequence through ycge_volume_camera_tick in THIS process (tests/test_gpu_volume_camera.py starts it with
    YCGE_CAMERA_HOST=1): one JSON line {scene: {seed: [[body words, info], ...]}}"""
    import json
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    out = {}
    for name in SCENES:
        sc, world, starts = make_scene(name)
        g = RaytraceRenderer(flatten(sc), 32, 16, 45.0, 1)
        w = abi.CameraWorld(*world)
        out[name] = {}
        for seed in SEEDS[name]:
            start, auto_placed, ticks = draw_sequence(seed, starts)
            b = new_body(start, auto_placed)
            rows = []
            for moves, dt_ms, run_update in ticks:
                info = g.CameraTick(b, w, moves, dt_ms, run_update)
                rows.append([[int(v) for v in body_words(b)], info])
            out[name][str(seed)] = rows
        g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    import sys
    if "--run-sequences" in sys.argv:
        _run_sequences_on_the_device()
