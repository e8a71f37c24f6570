"""VolumeScene's camera physics without a GPU: the restatement (tests/volume_camera_restatement.py) on scenes whose outcome is derived by
hand, and the library's stepper (csrc/ycge_camera_physics.h through ycge_test_camera_tick_host) held to the restatement bit for bit - in the
reference's serial order and in the device's window-and-commit order - over the oracle's Scene.Hit and over a synthetic one.

No device is touched: the hook takes Scene.Hit as a C callback.
"""
import ctypes as C
import hashlib
import struct

import numpy as np
import pytest

import volume_camera_cases as vc
import volume_camera_restatement as vr
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.scene import AmbientLight, Box, Material, Scene, flatten, vec3

F32, F64 = np.float32, np.float64
REST_Y = F32(F64(0.0) + F64(F32(1.7)) + F64(F32(0.1)))          # binary32 of ground + EyeHeight + GroundClearance over a floor at y = 0


@pytest.fixture(scope="module")
def hook(product_lib):
    assert hasattr(product_lib, "ycge_test_camera_tick_host")
    return vc.bind_hook(product_lib)


def hand_scene(*boxes):
    m = Material(vec3(0.7, 0.7, 0.7), 0.0, 0.0)
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.1)
    for lo, hi in boxes:
        s.Objects.append(Box(vec3(*lo), vec3(*hi), m, 0.0, 0.0))
    return s


FLOOR = ((-20, -1, -20), (20, 0, 20))


def camera_over(oracle, boxes, pos, auto_placed=True):
    sc = hand_scene(*boxes)
    o = oracle.OracleRenderer(sc, 16, 8, 1, None, flat=flatten(sc))
    return o, vr.VolumeCamera(vc.oracle_hit(o), pos, *vc.WORLD_BOXES, auto_placed=auto_placed)


# ------------------------------------------------------------------------------------------------ 1: outcomes derived by hand
def test_drop_comes_to_rest_on_the_floor(oracle):
    """from y = 3 over a floor whose top is y = 0: falls under 9.81 m/s^2, then rests at binary32(0 + 1.7f + 0.1f), grounded, velocity 0"""
    o, cam = camera_over(oracle, [FLOOR], (0.25, 3.0, -0.5))
    try:
        ys = []
        for _ in range(80):
            cam.tick([], 16.0)
            ys.append(cam.CameraPos[1])
            if cam.isGrounded: break
        assert cam.isGrounded and len(ys) > 10                  # (a fall of 1.2 takes ~0.5 s)
        assert all(b < a for a, b in zip(ys, ys[1:]))
        assert cam.CameraPos[1].view(np.uint32) == REST_Y.view(np.uint32) and cam.verticalVelocity == 0
        assert cam.CameraPos[0] == F32(0.25) and cam.CameraPos[2] == F32(-0.5)
        c = cam.tick([], 16.0)                                  # and stays
        assert cam.isGrounded and cam.CameraPos[1] == REST_Y and c["rays_committed"] == 8 + 5 + 5 + 32
    finally:
        o.close()


def test_walk_into_a_wall_stops_at_the_capsule_margin(oracle):
    """a wall whose face is x = 2: a move of 3 along +x from x = 0 ends 0.01 in front of it (LimitStepByRay's cand = t - 0.01), the micro-step
    after that is blocked; nothing else moves"""
    o, cam = camera_over(oracle, [FLOOR, ((2, 0, -5), (3, 4, 5))], (0.0, float(REST_Y), 0.0))
    try:
        c = cam.tick([(vr.MOVE_HORIZONTAL, 0, 3.0, 0.0)], 16.0, run_update=False)
        assert abs(float(cam.CameraPos[0]) - 1.99) < 1e-5
        assert cam.CameraPos[1] == REST_Y and cam.CameraPos[2] == 0
        assert c["blocked_steps"] == 1 and c["slides"] == 0 and c["micro_steps"] == int(1.99 / (0.65 * 0.35)) + 2
        assert c["rays_committed"] == 6 * c["micro_steps"]
    finally:
        o.close()


def test_oblique_walk_slides_along_the_wall(oracle):
    o, cam = camera_over(oracle, [FLOOR, ((2, 0, -9), (3, 4, 9))], (0.0, float(REST_Y), 0.0))
    try:
        k = 4.0 / np.sqrt(2.0)
        c = cam.tick([(vr.MOVE_HORIZONTAL, 0, k, k)], 16.0, run_update=False)
        assert c["slides"] >= 1 and c["blocked_steps"] == 0
        # the capsule's side rays (offset 0.65 across the heading) meet the wall before the centre does: x stops short of 1.99 and stays
        assert 1.0 < float(cam.CameraPos[0]) < 1.99 + 1e-5
        assert float(cam.CameraPos[2]) > 2.5                     # the whole length of 4 is used: what x lost, z got
    finally:
        o.close()


def test_start_inside_a_post_is_pushed_out_along_the_nearest_exit(oracle):
    """a post 0.2 x 0.22 thick around the camera: every embed probe (0.1625) hits, the nearest exit is +x at 0.08, so x = 0.02 + 0.08 + 0.02;
    the push-out then finds the post's face 0.02 behind and moves on by 0.63 + 0.01"""
    o, cam = camera_over(oracle, [FLOOR, ((-0.1, 0, -0.1), (0.1, 3, 0.12))], (0.02, float(REST_Y), 0.0))
    try:
        c = cam.tick([], 16.0)
        assert c["embedded_resolutions"] == 1 and c["push_outs"] >= 1
        assert abs(float(cam.CameraPos[0]) - 0.76) < 1e-5 and cam.CameraPos[2] == 0
        assert cam.isGrounded and cam.CameraPos[1] == REST_Y
    finally:
        o.close()


def test_below_the_fail_safe_goes_to_200(oracle):
    o, cam = camera_over(oracle, [FLOOR], (1.0, -11.0, 1.0))
    try:
        cam.verticalVelocity = F32(-3.0)
        c = cam.tick([], 16.0)
        assert c["fail_safes"] == 1 and cam.CameraPos[1] == F32(200.0) and cam.verticalVelocity == 0
    finally:
        o.close()


def test_first_tick_auto_places(oracle):
    """autoPlaced false: the fan from min(WorldHeight + 16, 4096) finds the floor, the camera stands on it, and Update returns early"""
    o, cam = camera_over(oracle, [FLOOR], (0.5, 50.0, 0.5), auto_placed=False)
    try:
        c = cam.tick([], 16.0)
        assert cam.autoPlaced and c["auto_placements"] == 1 and cam.CameraPos[1] == REST_Y and c["rays_committed"] == 8 + 5
        o2, cam2 = camera_over(oracle, [((30, -1, 30), (31, 0, 31))], (0.5, 50.0, 0.5), auto_placed=False)       # nothing below: WaterLevel + 1.7f + 4
        cam2.tick([], 16.0)
        assert cam2.CameraPos[1] == F32(4.0) + F32(1.7) + F32(4.0)
        o2.close()
    finally:
        o.close()


# ------------------------------------------------------------------------------------------------ 2, 3: drawn sequences over the oracle
@pytest.fixture(scope="module")
def references(oracle):
    """per scene: the oracle, its Scene.Hit, the world, the drawn sequences and the restatement's result after every tick - computed once"""
    out = {}
    for name in vc.SCENES:
        sc, world, starts = vc.make_scene(name)
        o = oracle.OracleRenderer(sc, 16, 8, 1, None, flat=flatten(sc))
        hit = vc.oracle_hit(o)
        seqs = {seed: vc.draw_sequence(seed, starts) for seed in vc.SEEDS[name]}
        refs = {seed: vc.run_restatement(hit, world, seq) for seed, seq in seqs.items()}
        out[name] = (o, hit, world, seqs, refs)
    yield out
    for o, *_ in out.values():
        o.close()


@pytest.mark.parametrize("name", vc.SCENES)
def test_sequences_reach_every_event(references, name):
    """what the seeds were chosen for, on the restatement alone: each scene's draws slide, push out, resolve an embedded start, snap to the
    ground, block a micro-step, auto-place and trip the fail-safe somewhere; and no move comes near the library's cap"""
    _, _, _, seqs, refs = references[name]
    total = dict.fromkeys(vc.EVENTS, 0)
    for seed, (ticks, cam) in refs.items():
        for _, counters in ticks:
            for k in total: total[k] += counters[k]
        assert cam.max_micro < abi.CAMERA_MAX_MICRO_STEPS // 4, (seed, cam.max_micro)
        for moves, dt_ms, _ in seqs[seed][2]:
            assert len(moves) <= abi.CAMERA_MAX_MOVES and 0.0 <= dt_ms <= 100.0
    assert all(v > 0 for v in total.values()), total


@pytest.mark.parametrize("windowed", [0, 1], ids=["serial", "windowed"])
@pytest.mark.parametrize("name", vc.SCENES)
def test_hook_matches_the_restatement(hook, references, name, windowed):
    """body after every tick bit for bit, rays_committed and every event counter equal; windowed: no fewer rays walked than committed"""
    _, hit, world, seqs, refs = references[name]
    walked = committed = 0
    for seed, (start, auto_placed, ticks) in seqs.items():
        b, w, cb = vc.new_body(start, auto_placed), abi.CameraWorld(*world), vc.c_callback(hit)
        for i, (moves, dt_ms, run_update) in enumerate(ticks):
            rc, info, msg = vc.tick_hook(hook, b, w, moves, dt_ms, run_update, cb, windowed)
            assert rc == abi.YCGE_OK, (seed, i, msg)
            vc.assert_same(b, info, refs[seed][0][i][0], refs[seed][0][i][1], (name, seed, i))
            assert info["rays_walked"] >= info["rays_committed"] and info["windows"] <= info["rays_committed"]
            if not windowed:
                assert info["rays_walked"] == info["rays_committed"] == info["windows"]
            walked += info["rays_walked"]; committed += info["rays_committed"]
        assert cb.py.calls > 0
    if windowed:
        assert walked > committed                                            # some window was cut by a ray that changed the state


# ------------------------------------------------------------------------------------------------ 4: a synthetic pure Scene.Hit
def hash_hit(salt, p_hit):
    """a pure function of the ray's bits: hit or not, t inside the interval, a unit normal - far more hits than a scene gives"""
    def hit(o, d, tmin, tmax):
        h = hashlib.blake2b(struct.pack("<8f", *o, *d, tmin, tmax) + salt, digest_size=16).digest()
        u = np.frombuffer(h, np.uint32).astype(np.float64) / 2.0 ** 32
        if u[0] >= p_hit: return None
        hi = min(float(tmax), float(tmin) + 1.5)
        t = F32(float(tmin) + u[1] * (hi - float(tmin)))
        a, e = 2.0 * np.pi * u[2], (u[3] - 0.5) * 2.0
        r = np.sqrt(max(0.0, 1.0 - e * e))
        return t, (F32(r * np.cos(a)), F32(e), F32(r * np.sin(a)))
    return hit


@pytest.mark.parametrize("p_hit", [0.15, 0.5, 0.9])
def test_windowed_equals_serial_on_a_synthetic_hit(hook, p_hit):
    world = vc.WORLD_BOXES
    hit = hash_hit(struct.pack("<d", p_hit), p_hit)
    total_walked = total_committed = 0
    for seed in range(6):
        start, auto_placed, ticks = vc.draw_sequence(100 + seed, [(0.0, 2.0, 0.0), (1.0, -20.0, 3.0)], n_ticks=6)
        cam = vr.VolumeCamera(hit, start, *world, auto_placed=auto_placed)
        bodies = [vc.new_body(start, auto_placed) for _ in range(2)]
        w = abi.CameraWorld(*world)
        for i, (moves, dt_ms, run_update) in enumerate(ticks):
            counters = cam.tick(moves, dt_ms, run_update)
            assert cam.max_micro < abi.CAMERA_MAX_MICRO_STEPS
            want = vc.restatement_words(cam)
            for windowed in (0, 1):
                rc, info, msg = vc.tick_hook(hook, bodies[windowed], w, moves, dt_ms, run_update, vc.c_callback(hit), windowed)
                assert rc == abi.YCGE_OK, (seed, i, msg)
                vc.assert_same(bodies[windowed], info, want, counters, (p_hit, seed, i, windowed))
                assert info["rays_walked"] >= info["rays_committed"]
                if windowed:
                    total_walked += info["rays_walked"]; total_committed += info["rays_committed"]
            assert bytes(bodies[0]) == bytes(bodies[1])
    assert total_walked > total_committed


# ------------------------------------------------------------------------------------------------ 5: refusals and the cap
def test_refusals_leave_the_body_alone(hook):
    miss = vc.c_callback(lambda o, d, tmin, tmax: None)
    w = abi.CameraWorld(*vc.WORLD_BOXES)
    good = [(vr.MOVE_HORIZONTAL, 0, 0.1, 0.0)]
    nan, inf = float("nan"), float("inf")

    def call(body, world, moves, n, dt=16.0, null_moves=False):
        recs = (abi.CameraMove * max(1, len(moves)))(*[abi.CameraMove(*m) for m in moves])
        msg = C.create_string_buffer(256)
        info = abi.CameraTickInfo()
        rc = hook.ycge_test_camera_tick_host(C.byref(body) if body is not None else None, C.byref(world) if world is not None else None,
                                             None if null_moves else recs, n, dt, 1, C.byref(info), miss, None, 1, msg, 256)
        return rc, msg.value.decode()

    b = vc.new_body((0.0, 2.0, 0.0), True)
    before = bytes(b)
    assert call(None, w, good, 1)[0] == abi.YCGE_ERR_INVALID_ARG and call(b, None, good, 1)[0] == abi.YCGE_ERR_INVALID_ARG
    for n in (-1, abi.CAMERA_MAX_MOVES + 1):
        rc, msg = call(b, w, good, n)
        assert rc == abi.YCGE_ERR_INVALID_ARG and "n_moves" in msg
    assert call(b, w, good, 1, null_moves=True)[0] == abi.YCGE_ERR_INVALID_ARG
    for dt in (nan, inf, -inf):
        assert call(b, w, good, 1, dt=dt)[0] == abi.YCGE_ERR_INVALID_ARG
    bad_moves = [((vr.MOVE_HORIZONTAL, 0, 64.5, 0.0), "longer"), ((vr.MOVE_HORIZONTAL, 0, 46.0, 46.0), "longer"), ((vr.MOVE_VERTICAL, 0, -64.5, 0.0), "longer"),
                 ((4, 0, 0.0, 0.0), "kind"), ((-1, 0, 0.0, 0.0), "kind"), ((vr.MOVE_HORIZONTAL, 0, nan, 0.0), "finite"), ((vr.MOVE_VERTICAL, 0, inf, 0.0), "finite"),
                 ((vr.MOVE_JUMP, 0, 0.0, nan), "finite")]
    for m, word in bad_moves:
        rc, msg = call(b, w, good + [m], 2)
        assert rc == abi.YCGE_ERR_INVALID_ARG and "move 1:" in msg and word in msg, (m, msg)
    assert call(b, w, good + [(vr.MOVE_HORIZONTAL, 0, 64.0, 0.0), (vr.MOVE_VERTICAL, 0, 64.0, 0.0)], 3)[0] == abi.YCGE_OK       # the limit itself is accepted
    b = vc.new_body((0.0, 2.0, 0.0), True)
    for field, v in (("pos", nan), ("vertical_velocity", inf), ("shift_hold_timer", nan), ("repel_vel", -inf)):
        bb = vc.new_body((0.0, 2.0, 0.0), True)
        if field in ("pos", "repel_vel"): getattr(bb, field)[1] = v
        else: setattr(bb, field, v)
        snap = bytes(bb)
        rc, msg = call(bb, w, good, 1)
        assert rc == abi.YCGE_ERR_INVALID_ARG and "body" in msg and bytes(bb) == snap
    assert call(b, abi.CameraWorld(nan, 4.0, 1.0), good, 1)[0] == abi.YCGE_ERR_INVALID_ARG
    assert bytes(b) == before
    msg = C.create_string_buffer(64)
    assert hook.ycge_test_camera_tick_host(C.byref(b), C.byref(w), None, 0, 16.0, 1, None, C.cast(None, abi.CAMERA_HIT_FN), None, 0, msg, 64) == abi.YCGE_ERR_INVALID_ARG


@pytest.mark.parametrize("windowed", [0, 1], ids=["serial", "windowed"])
def test_a_slide_that_never_ends_reaches_the_cap(hook, windowed):
    """a corner that blocks every capsule ray 0.05 ahead with a normal at 45 degrees to the heading: each micro-step advances 0.04, slides, and
    adds its residual back (:275) - `remaining` grows, the reference would never return.  The library stops at its cap"""
    def corner(o, d, tmin, tmax):
        if d[1] != 0: return None                               # (the update's vertical fans: open air)
        l = np.sqrt(float(d[0]) ** 2 + float(d[2]) ** 2)
        dx, dz = float(d[0]) / l, float(d[2]) / l
        s = np.sqrt(0.5)
        return F32(0.05), (F32(-(dx * s - dz * s)), F32(0.0), F32(-(dx * s + dz * s)))
    b = vc.new_body((0.0, 2.0, 0.0), True)
    before = bytes(b)
    rc, info, msg = vc.tick_hook(hook, b, abi.CameraWorld(*vc.WORLD_BOXES), [(vr.MOVE_JUMP, 0, 0.0, 0.0), (vr.MOVE_HORIZONTAL, 0, 1.0, 0.0)], 16.0, True,
                                 vc.c_callback(corner), windowed)
    assert rc == abi.YCGE_ERR_UNSUPPORTED, msg
    assert "move 1:" in msg and str(abi.CAMERA_MAX_MICRO_STEPS) in msg and "horizontal" in msg
    assert bytes(b) == before and all(v == 0 for v in info.values())
