"""-m gpu: many bodies of the voxel world a tick in one launch, each with its own shape (ycge_volume_bodies_tick, k_bodies_tick in
csrc/ycge_camera.hip), against the restatement (tests/volume_camera_restatement.py) over the oracle's Scene.Hit - every body after every
tick bit for bit, rays_committed and every event counter equal - against the single tick (ycge_volume_camera_tick) body by body, and
against the batch hook over the oracle; on both kernel instances (a voxel world, analytic boxes without a grid) and on a scene whose
traversal stack spills.  No test here reaches a cap: status 1..3 on the device rests on the stepper shared with the hook
(tests/test_volume_bodies_cpu.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_util as pu
import volume_bodies_cases as bc
import volume_camera_cases as vc
import volume_camera_restatement as vr
from yetanotherconsolegameengine_amd import abi, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer, VolumeBodies
from yetanotherconsolegameengine_amd.scene import AmbientLight, Box, Material, Mesh, PointLight, Scene, flatten, vec3

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def references(oracle):
    """per scene: the scene, the world, the start positions, and for the two batches of tests/test_volume_bodies_cpu.py - every committed
    seed with the reference's shape; the (seed, shape) pairs - the sequences, the shape names and the restatement's result after every
    tick over the oracle.  Computed once"""
    out = {}
    for name in vc.SCENES:
        sc, world, starts = vc.make_scene(name)
        o = oracle.OracleRenderer(sc, 16, 8, 1, None, flat=flatten(sc))
        hit = vc.oracle_hit(o)
        plain = bc.batch_sequences(vc.SEEDS[name], starts)
        shaped = bc.batch_sequences([seed for seed, _ in bc.PAIRS[name]], starts)
        names = [shape for _, shape in bc.PAIRS[name]]
        out[name] = {"scene": sc, "world": world, "starts": starts,
                     "plain": (plain, ["default"] * len(plain), [bc.restate(hit, world, seq)[0] for seq in plain]),
                     "shaped": (shaped, names, [bc.restate(hit, world, seq, shape)[0] for seq, shape in zip(shaped, names)])}
        o.close()
    return out


def moves_of(rows):
    return [abi.CameraMove(int(k), int(s), float(a), float(b)) for k, s, a, b in rows]


def run_batch(g, ref, which, shapes):
    """a batch through ycge_volume_bodies_tick, held to the restatement after every tick: [[body bytes]] per tick"""
    seqs, names, refs = ref[which]
    bodies = bc.body_array(seqs)
    w = abi.CameraWorld(*ref["world"])
    rows = []
    walked = committed = 0
    for k in range(len(seqs[0][2])):
        _, dt_ms, run_update = seqs[0][2][k]
        results, infos = g.BodiesTick(bodies, w, [s[2][k][0] for s in seqs], dt_ms, run_update, bc.shape_array(names) if shapes else None)
        assert results == [(0, -1)] * len(seqs), (k, results)
        for i in range(len(seqs)):
            bc.assert_body(bodies[i], infos[i], refs[i][k], (which, i, names[i], k))
            assert infos[i]["rays_walked"] >= infos[i]["rays_committed"] >= infos[i]["windows"]
            walked += infos[i]["rays_walked"]; committed += infos[i]["rays_committed"]
        rows.append([bytes(b) for b in bodies])
    assert walked > committed
    return rows


# ------------------------------------------------------------------------------------------------ 1: every committed seed, one batch a scene
@pytest.mark.parametrize("name", vc.SCENES)
def test_device_batch_matches_the_restatement_and_the_single_tick(product_lib, references, name):
    ref = references[name]
    g = RaytraceRenderer(flatten(ref["scene"]), 32, 16, 45.0, 1)
    try:
        rows = run_batch(g, ref, "plain", shapes=False)
        seqs = ref["plain"][0]
        w = abi.CameraWorld(*ref["world"])
        for i, (start, auto_placed, ticks) in enumerate(seqs):                 # body by body: ycge_volume_camera_tick on the same context
            b = vc.new_body(start, auto_placed)
            for k, (moves, dt_ms, run_update) in enumerate(ticks):
                g.CameraTick(b, w, moves_of(moves), dt_ms, run_update)
                assert bytes(b) == rows[k][i], (name, i, k)
    finally:
        g.close()


def test_host_route_matches_the_restatement(product_lib, references):
    """the same batches with the stepper on the host, a round one batch of scene queries: a child process made with YCGE_CAMERA_HOST=1"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(bc.__file__)))
    path = os.pathsep.join([root, os.path.join(root, "tests")] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else []))
    env = dict(os.environ, YCGE_CAMERA_HOST="1", PYTHONPATH=path)
    r = subprocess.run([sys.executable, bc.__file__, "--run-batches"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for name in vc.SCENES:
        seqs, _, refs = references[name]["plain"]
        assert len(got[name]) == len(seqs[0][2])
        for k, row in enumerate(got[name]):
            assert len(row) == len(seqs)
            for i, (words, status, info) in enumerate(row):
                want, counters = refs[i][k]
                assert status == 0 and np.array_equal(np.array(words, np.uint32), want), (name, i, k)
                for key in ("rays_committed",) + vc.EVENTS:
                    assert info[key] == counters[key], (name, i, k, key)


# ------------------------------------------------------------------------------------------------ 2: shapes
@pytest.mark.parametrize("name", vc.SCENES)
def test_shapes_on_the_device(product_lib, references, name):
    """small, large and floaty bodies mixed with default ones, one batch a scene: the pairs of the CPU file"""
    g = RaytraceRenderer(flatten(references[name]["scene"]), 32, 16, 45.0, 1)
    try:
        run_batch(g, references[name], "shaped", shapes=True)
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ 3: many workgroups
@pytest.mark.parametrize("name", vc.SCENES)
def test_many_workgroups_equal_their_solo_ticks(product_lib, references, name):
    """130 bodies - the scene's sequences, their first three ticks, repeated from shifted starts, so the move lists are uneven - in one launch
    of 130 workgroups: body i is what ycge_volume_camera_tick makes of it alone.  Then n = 1 and n = 2"""
    ref = references[name]
    base = ref["plain"][0]
    seqs = []
    for i in range(130):
        (x, y, z), auto_placed, ticks = base[i % len(base)]
        j = i // len(base)
        seqs.append(((x + 0.11 * j, y, z - 0.07 * j), auto_placed, ticks[:3]))
    w = abi.CameraWorld(*ref["world"])
    g = RaytraceRenderer(flatten(ref["scene"]), 32, 16, 45.0, 1)
    try:
        solo = []
        for start, auto_placed, ticks in seqs:
            b = vc.new_body(start, auto_placed)
            rows = []
            for moves, dt_ms, run_update in ticks:
                info = g.CameraTick(b, w, moves_of(moves), dt_ms, run_update)
                rows.append((bytes(b), info))
            solo.append(rows)
        for pick in (list(range(130)), [17], [40, 93]):
            bodies = bc.body_array([seqs[i] for i in pick])
            for k in range(3):
                _, dt_ms, run_update = seqs[0][2][k]
                results, infos = g.BodiesTick(bodies, w, [seqs[i][2][k][0] for i in pick], dt_ms, run_update)
                assert results == [(0, -1)] * len(pick)
                for at, i in enumerate(pick):
                    assert bytes(bodies[at]) == solo[i][k][0] and infos[at] == solo[i][k][1], (name, len(pick), i, k)
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ 4: a scene whose stack spills
def heightfield_scene():
    """a ground mesh of 48 x 48 cells (4 608 triangles) over x, z in [-12, 12] with a few boxes standing on it"""
    m = Material(vec3(0.6, 0.7, 0.5), 0.0, 0.0)
    n = 48
    xs = np.linspace(-12.0, 12.0, n + 1)
    X, Z = np.meshgrid(xs, xs, indexing="ij")
    Y = 1.2 * np.sin(0.5 * X) * np.cos(0.4 * Z) + 0.3 * np.sin(1.3 * X + 0.7 * Z)
    P = np.stack([X, Y, Z], axis=-1).astype(F32)
    a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
    tris = np.concatenate([np.stack([a, c, b], axis=2).reshape(-1, 3, 3), np.stack([a, d, c], axis=2).reshape(-1, 3, 3)]).astype(F32)
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.1)
    s.Lights.append(PointLight(vec3(0.0, 9.0, 0.0), vec3(1, 1, 1), 60.0))
    s.Objects.append(Mesh(np.ascontiguousarray(tris), m))
    for lo, hi in (((-3.0, -2.0, -3.0), (-1.5, 4.0, -1.0)), ((2.0, -2.0, 1.0), (4.0, 3.0, 2.5)), ((-8.0, -2.0, 5.0), (-6.5, 5.0, 7.0)), ((6.0, -2.0, -7.0), (8.0, 4.0, -5.5)),
                   ((0.5, -2.0, -9.0), (1.5, 4.0, -8.0))):
        s.Objects.append(Box(vec3(*lo), vec3(*hi), m, 0.0, 0.0))
    return s


def test_a_scene_with_spill_levels(product_lib, oracle):
    """40 bodies walk the heightfield for 5 ticks: every workgroup has its own columns of the spill area (max(1, levels) x 64 * n entries,
    lane l of workgroup b at b * 64 + l).  Held against the solo ticks and against the hook over the oracle.  (That a walk reached the
    spilled levels is not shown here; the sizing is checked by reading.)"""
    sc = heightfield_scene()
    world = (16.0, 4.0, 1.0)
    w = abi.CameraWorld(*world)
    rng = np.random.default_rng(41)
    n = 40
    starts = [(float(rng.uniform(-10, 10)), float(rng.uniform(2.5, 6.0)), float(rng.uniform(-10, 10))) for _ in range(n)]
    autos = [bool(i % 5 != 4) for i in range(n)]
    names = [("default", "small", "large", "floaty")[i % 4] for i in range(n)]
    ticks = []
    for k in range(5):
        per_body = []
        for i in range(n):
            ms = []
            for _ in range(int(rng.integers(0, 3)) if k else 0):
                ang, step = rng.uniform(-np.pi, np.pi), rng.uniform(0.1, 1.5)
                ms.append((vr.MOVE_HORIZONTAL, 0, float(F32(np.sin(ang) * step)), float(F32(-np.cos(ang) * step))) if rng.random() < 0.8 else (vr.MOVE_JUMP, 0, 0.0, 0.0))
            per_body.append(ms)
        ticks.append((per_body, 33.0 if k else 16.0))
    g = RaytraceRenderer(flatten(sc), 32, 16, 45.0, 1)
    o = oracle.OracleRenderer(sc, 16, 8, 1, None, flat=flatten(sc))
    try:
        depth = g.scene_bvh_stats()["max_depth"] + 4 + g.mesh_bvh_stats()["max_depth"] + 2
        assert depth > 12, depth                                                # YCGE_LDS_STACK_LEVELS: the context's spill_levels is depth - 12 > 0
        hook = vc.bind_hook(product_lib)
        cb = vc.c_callback(vc.oracle_hit(o))
        seqs = [(starts[i], autos[i], None) for i in range(n)]
        on_device, over_oracle = bc.body_array(seqs), bc.body_array(seqs)
        alone = [bc.body_array([s]) for s in seqs]
        shapes = bc.shape_array(names)
        for k, (per_body, dt_ms) in enumerate(ticks):
            results, infos = g.BodiesTick(on_device, w, per_body, dt_ms, True, shapes)
            assert results == [(0, -1)] * n, (k, results)
            rc, hres, hinfos, msg = bc.tick_hook(hook, over_oracle, shapes, w, per_body, dt_ms, True, cb, 1)
            assert rc == abi.YCGE_OK and hres == results, msg
            for i in range(n):
                r1, i1 = g.BodiesTick(alone[i], w, [per_body[i]], dt_ms, True, bc.shape_array([names[i]]))
                assert r1 == [(0, -1)] and bytes(alone[i][0]) == bytes(on_device[i]) and i1[0] == infos[i], (k, i, "solo")
                assert bytes(over_oracle[i]) == bytes(on_device[i]), (k, i, names[i], list(on_device[i].pos), list(over_oracle[i].pos))
                for key in ("rays_committed", "rays_walked", "windows") + vc.EVENTS:
                    assert infos[i][key] == hinfos[i][key], (k, i, key)
        assert any(b.is_grounded for b in on_device)
    finally:
        o.close(); g.close()


# ------------------------------------------------------------------------------------------------ 5: frames unaffected
POSES = [((0.0, 1.0, 0.0), 0.0, 0.0), ((0.0, 1.0, 0.0), 0.0, 0.0), ((0.05, 1.0, 0.1), 0.02, -0.01), ((0.05, 1.0, 0.1), 0.02, -0.01)]


def _crowd(world, origin, n=6):
    crowd = VolumeBodies(*world)
    for i in range(n):
        crowd.add((origin[0] + 0.4 * i, origin[1], origin[2] - 0.3 * i), shape=[None, bc.SHAPES["small"], bc.SHAPES["large"]][i % 3], auto_placed=True)
    return crowd


def _move(g, crowd, k):
    for i, body in enumerate(crowd.bodies):
        if (i + k) % 3: body.forward(0.3 * k + i, 0.016)
        if (i + k) % 2: body.jump()
    results, _ = crowd.tick(g, 16.0)
    assert all(status == 0 for status, _ in results)


def test_frames_unaffected_synchronous(product_lib):
    """the same frames, bit for bit - SDR, TAA history, RNG state - with bodies ticks between them and without"""
    sc, w, h, ss, pose = scenes.config_scene(2)
    flat = flatten(sc)
    out = []
    for with_ticks in (False, True):
        g = RaytraceRenderer(flat, 160, 45, 45.0, 1, capture_debug=True)
        crowd = _crowd((16.0, 4.0, 1.0), (0.0, 3.0, 0.0))
        frames = []
        for k, (p, y, pt) in enumerate(POSES):
            g.SetCamera(p, y, pt)
            if with_ticks: _move(g, crowd, k)
            sdr = g.TryFlipAndBlit(want_sdr=True)
            if with_ticks: _move(g, crowd, 10 + k)
            frames.append((sdr, g.read(abi.BUF_TAA_HISTORY), g.read(abi.BUF_RNG_STATE), int(g.stats.frame)))
        out.append(frames)
        g.close()
    for a, b in zip(*out):
        assert pu.mismatch_count(a[0], b[0]) == 0 and pu.mismatch_count(a[1], b[1]) == 0 and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_frames_unaffected_in_flight(product_lib):
    """frames in flight: a bodies tick between two of them does not join the one in flight - frames_outstanding stays 1 - and the frames are
    the ones the same sequence without ticks gives"""
    sc, w, h, ss, pose = scenes.config_scene(5, small=True, t01=0.5)
    flat = flatten(sc)
    p0 = pose["pos"]
    out = []
    for with_ticks in (False, True):
        g = RaytraceRenderer(flat, 160, 45, pose.get("fov", 45.0), 1)
        crowd = _crowd(vc.WORLD5, p0)
        sdrs = []
        for k in range(4):
            g.SetCamera((p0[0] + 0.01 * k, p0[1], p0[2]), pose["yaw"], pose["pitch"])
            a = g.RenderAsync(sdr_slot=k % 2)
            if with_ticks:
                _move(g, crowd, k)
                assert g.flight_info()["frames_outstanding"] == 1
            g.Wait()
            sdrs.append(a.copy())
        out.append((sdrs, g.read(abi.BUF_TAA_HISTORY)))
        g.close()
    for a, b in zip(out[0][0], out[1][0]):
        assert pu.mismatch_count(a, b) == 0
    assert pu.mismatch_count(out[0][1], out[1][1]) == 0


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals(product_lib, oracle):
    L = product_lib
    w = abi.CameraWorld(*vc.WORLD_BOXES)
    N = 3

    def arrays():
        b = (abi.CameraBody * N)(*[vc.new_body((0.5 * i, 2.0, 0.0), True) for i in range(N)])
        m, f = bc.pack_moves([[(vr.MOVE_HORIZONTAL, 0, 0.1, 0.0)], [(vr.MOVE_HORIZONTAL, 0, 0.1, 0.0), (vr.MOVE_VERTICAL, 0, 0.1, 0.0)], []])
        r = (abi.BodyResult * N)()
        i = (abi.CameraTickInfo * N)()
        C.memset(r, 0xAB, C.sizeof(r)); C.memset(i, 0xAB, C.sizeof(i))
        return b, m, f, r, i

    g0 = RaytraceRenderer(None, 16, 8, 45.0, 1)
    try:
        b, m, f, r, i = arrays()
        before = bytes(b)
        assert L.ycge_volume_bodies_tick(g0.ctx, b, None, N, C.byref(w), m, f, 16.0, 1, r, i) == abi.YCGE_ERR_NO_SCENE
        assert L.ycge_volume_bodies_tick(g0.ctx, None, None, 0, None, None, None, 16.0, 1, None, None) == abi.YCGE_ERR_NO_SCENE
        assert bytes(b) == before and bytes(r) == b"\xab" * C.sizeof(r)
    finally:
        g0.close()
    sc = vc.box_scene()
    o = oracle.OracleRenderer(sc, 16, 8, 1, None, flat=flatten(sc))
    g = RaytraceRenderer(flatten(sc), 32, 16, 45.0, 1, devices=[0, 0])
    try:
        def refused(ctx=None, n=N, null=(), poke=None, shapes=None, dt=16.0, status=abi.YCGE_ERR_INVALID_ARG):
            b, m, f, r, i = arrays()
            if poke: poke(b, m, f)
            before = bytes(b)
            args = {"bodies": b, "world": C.byref(w), "moves": m, "first": f, "results": r}
            for k in null: args[k] = None
            ctx = g.ctx if ctx is None else ctx
            rc = L.ycge_volume_bodies_tick(ctx, args["bodies"], shapes, n, args["world"], args["moves"], args["first"], dt, 1, args["results"], i)
            assert rc == status, L.ycge_last_error(ctx)
            assert bytes(b) == before and bytes(r) == b"\xab" * C.sizeof(r) and bytes(i) == b"\xab" * C.sizeof(i)
            return L.ycge_last_error(ctx)

        b, m, f, r, i = arrays()
        assert L.ycge_volume_bodies_tick(None, b, None, N, C.byref(w), m, f, 16.0, 1, r, i) == abi.YCGE_ERR_INVALID_ARG
        peer = C.c_void_p(L.ycge_debug_peer_context(g.ctx, 0))
        assert peer.value and b"driven by their root" in refused(ctx=peer)
        for n in (-1, abi.BODIES_MAX + 1):
            assert b"YCGE_BODIES_MAX" in refused(n=n)
        for null in ("bodies", "world", "results", "first"):
            assert refused(null=(null,)).startswith(b"ycge_volume_bodies_tick: NULL")
        assert b"body 0: NULL moves" in refused(null=("moves",))
        assert b"delta_time_ms" in refused(dt=float("nan"))

        def first(*vals):
            return lambda b, m, f: f.__setitem__(slice(None), vals)
        assert b"body 0:" in refused(poke=first(1, 1, 3, 3)) and b"body 1: move_first decreases" in refused(poke=first(0, 2, 1, 3))
        assert b"body 1: more than YCGE_CAMERA_MAX_MOVES" in refused(poke=first(0, 1, 2 + abi.CAMERA_MAX_MOVES, 2 + abi.CAMERA_MAX_MOVES))
        for (kind, a), word in (((0, 65.0), b"longer"), ((1, -65.0), b"longer"), ((7, 0.0), b"kind"), ((0, float("inf")), b"finite")):
            def poke(b, m, f, kind=kind, a=a):
                m[2].kind, m[2].a = kind, a                                    # body 1's moves are m[1], m[2]: its own move 1
            msg = refused(poke=poke)
            assert b"body 1: move 1:" in msg and word in msg, msg

        def nan_body(b, m, f):
            b[2].pos[1] = float("nan")
        assert b"body 2: a field of the body" in refused(poke=nan_body)
        for field, v in (("eye_height", float("nan")), ("collision_radius", 0.0), ("probe_radius", -0.1), ("gravity_accel", 0.0), ("ground_clearance", -0.1),
                         ("jump_speed", -1.0), ("eye_height", 65.0), ("collision_radius", 64.5)):
            s = bc.shape_array(["default", "small", "large"])
            setattr(s[1], field, v)
            msg = refused(shapes=s)
            assert b"body 1:" in msg and b"shape" in msg, (field, msg)
        # n = 0 with a scene: fine, nothing needed; and the context is usable and right afterwards (the root of a two-device context answers)
        assert L.ycge_volume_bodies_tick(g.ctx, None, None, 0, None, None, None, 16.0, 1, None, None) == abi.YCGE_OK
        b, m, f, r, i = arrays()
        rows = [[(vr.MOVE_HORIZONTAL, 0, 0.1, 0.0)], [(vr.MOVE_HORIZONTAL, 0, 0.1, 0.0), (vr.MOVE_VERTICAL, 0, 0.1, 0.0)], []]
        results, infos = g.BodiesTick(b, w, rows, 16.0)
        assert results == [(0, -1)] * N
        for k in range(N):
            cam = vr.VolumeCamera(vc.oracle_hit(o), (0.5 * k, 2.0, 0.0), *vc.WORLD_BOXES, auto_placed=True)
            counters = cam.tick(rows[k], 16.0)
            vc.assert_same(b[k], infos[k], vc.restatement_words(cam), counters, ("after the refusals", k))
        g.TryFlipAndBlit()
    finally:
        o.close(); g.close()
