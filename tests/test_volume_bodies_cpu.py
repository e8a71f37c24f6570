"""Many bodies of the voxel world a tick, each with its own shape, without a GPU: the batch hook (ycge_test_bodies_tick_host - the stepper of
csrc/ycge_camera_physics.h with a ycge_body_shape, the refusals and the per-body results of ycge_volume_bodies_tick) held to the restatement
(tests/volume_camera_restatement.py, its six size constants patched for a non-default shape) bit for bit, in the reference's serial order
and in the device's window-and-commit order, over the oracle's Scene.Hit and over a synthetic one.

No device is touched: the hook takes Scene.Hit as a C callback.
"""
import ctypes as C

import numpy as np
import pytest

import volume_bodies_cases as bc
import volume_camera_cases as vc
import volume_camera_restatement as vr
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.scene import flatten

F32 = np.float32
ORDERS = pytest.mark.parametrize("windowed", [0, 1], ids=["serial", "windowed"])


@pytest.fixture(scope="module")
def hook(product_lib):
    assert hasattr(product_lib, "ycge_test_bodies_tick_host")
    return vc.bind_hook(product_lib)


@pytest.fixture(scope="module")
def references(oracle):
    """per scene: the oracle's Scene.Hit, the world, and for the two batches - every committed seed with the reference's shape; the (seed,
    shape) pairs - the sequences, the shape names and the restatement's result after every tick.  Computed once"""
    out, oracles = {}, []
    for name in vc.SCENES:
        sc, world, starts = vc.make_scene(name)
        o = oracle.OracleRenderer(sc, 16, 8, 1, None, flat=flatten(sc))
        oracles.append(o)
        hit = vc.oracle_hit(o)
        plain = bc.batch_sequences(vc.SEEDS[name], starts)
        shaped = bc.batch_sequences([seed for seed, _ in bc.PAIRS[name]], starts)
        names = [shape for _, shape in bc.PAIRS[name]]
        out[name] = {"hit": hit, "world": world,
                     "plain": (plain, ["default"] * len(plain), [bc.restate(hit, world, seq) for seq in plain]),
                     "shaped": (shaped, names, [bc.restate(hit, world, seq, shape) for seq, shape in zip(shaped, names)])}
    yield out
    for o in oracles:
        o.close()


def run_batch(hook, ref, which, windowed, shapes="own", ticks=None, order=None):
    """the batch `which` of a scene through the hook, tick by tick: [(bodies bytes, results, infos)] after every tick; held to the restatement
    when check"""
    seqs, names, refs = ref[which]
    order = list(range(len(seqs))) if order is None else order
    seqs, names, refs = [seqs[i] for i in order], [names[i] for i in order], [refs[i] for i in order]
    bodies = bc.body_array(seqs)
    sh = None if shapes is None else bc.shape_array(names)
    w, cb = abi.CameraWorld(*ref["world"]), vc.c_callback(ref["hit"])
    rows = []
    for k in range(len(seqs[0][2]) if ticks is None else ticks):
        _, dt_ms, run_update = seqs[0][2][k]
        rc, results, infos, msg = bc.tick_hook(hook, bodies, sh, w, [s[2][k][0] for s in seqs], dt_ms, run_update, cb, windowed)
        assert rc == abi.YCGE_OK, (k, msg)
        assert results == [(0, -1)] * len(seqs), (k, results)
        for i in range(len(seqs)):
            bc.assert_body(bodies[i], infos[i], refs[i][0][k], (which, order[i], names[i], k))
            assert infos[i]["rays_walked"] >= infos[i]["rays_committed"] and (windowed or infos[i]["rays_walked"] == infos[i]["rays_committed"])
        rows.append(([bytes(b) for b in bodies], results, infos))
    assert cb.py.calls > 0
    return rows


# ------------------------------------------------------------------------------------------------ 1: every committed seed, one batch a scene
@ORDERS
@pytest.mark.parametrize("name", vc.SCENES)
def test_batch_matches_the_restatement(hook, references, name, windowed):
    """7 bodies on the voxel world, 8 on the boxes, 10 ticks: every body and every counter after every tick is the restatement's"""
    seqs = references[name]["plain"][0]
    assert len(seqs) == len(vc.SEEDS[name]) and len(seqs[0][2]) == 10
    counts = {len(s[2][k][0]) for s in seqs for k in range(10)}
    assert 0 in counts and len(counts) >= 3                                   # uneven move lists, some empty
    assert any(len({len(s[2][k][0]) for s in seqs}) > 1 for k in range(10))
    rows = run_batch(hook, references[name], "plain", windowed, shapes=None)
    if windowed:
        assert sum(i["rays_walked"] for _, _, infos in rows for i in infos) > sum(i["rays_committed"] for _, _, infos in rows for i in infos)


# ------------------------------------------------------------------------------------------------ 2: shapes
@pytest.mark.parametrize("name", vc.SCENES)
def test_pairs_reach_the_events_and_stay_off_the_cap(references, name):
    """what the (seed, shape) pairs were chosen for, on the restatement alone: no move comes near the library's cap"""
    seqs, names, refs = references[name]["shaped"]
    assert {"small", "large", "floaty", "default"} <= set(names)
    for seq, shape, (ticks, cam) in zip(seqs, names, refs):
        assert cam.max_micro < abi.CAMERA_MAX_MICRO_STEPS // 4, (shape, cam.max_micro)


@pytest.mark.parametrize("shape", ["small", "large", "floaty"])
def test_each_shape_shows_the_events(references, shape):
    """... and each shape shows, somewhere in its sequences of both scenes, a blocked micro-step, a push-out and a ground snap"""
    total = dict.fromkeys(("blocked_steps", "push_outs", "ground_snaps"), 0)
    for name in vc.SCENES:
        seqs, names, refs = references[name]["shaped"]
        assert shape in names                                                 # (sequences of BOTH scenes)
        for s, (ticks, _) in zip(names, refs):
            if s == shape:
                for _, counters in ticks:
                    for k in total: total[k] += counters[k]
    assert all(v > 0 for v in total.values()), (shape, total)


def test_a_shape_changes_the_outcome(references):
    """(the patched restatement is not the default one in disguise: a drop from y = 5 onto the boxes' floor, ten quiet ticks of 100 ms - the
    default body lands at 1.8, the small one at 0.95, the large one at 2.7, the floaty one is still falling)"""
    ref = references["boxes"]
    seq = ((0.3, 5.0, 0.2), True, [([], 100.0, True)] * 10)
    ends = {shape: bc.restate(ref["hit"], ref["world"], seq, shape)[0][-1][0] for shape in bc.SHAPES}
    ys = {shape: float(words.view(F32)[1]) for shape, words in ends.items()}
    assert abs(ys["default"] - 1.8) < 1e-5 and abs(ys["small"] - 0.95) < 1e-5 and abs(ys["large"] - 2.7) < 1e-5 and 3.0 < ys["floaty"] < 5.0, ys


@ORDERS
@pytest.mark.parametrize("name", vc.SCENES)
def test_shapes_batch_matches_the_restatement(hook, references, name, windowed):
    """small, large and floaty bodies mixed with default ones in one batch, each against the restatement with its six globals patched"""
    run_batch(hook, references[name], "shaped", windowed)


@pytest.mark.parametrize("name", vc.SCENES)
def test_null_shapes_are_the_default_shape(hook, references, name):
    a = run_batch(hook, references[name], "plain", 1, shapes=None, ticks=4)
    b = run_batch(hook, references[name], "plain", 1, shapes="own", ticks=4)            # an explicit array of YCGE_BODY_SHAPE_DEFAULT
    assert a == b
    d = abi.BodyShape(*abi.BODY_SHAPE_DEFAULT)
    assert bytes(d) == np.array([1.7, 0.65, 0.35, 0.10, 4.8, 9.81], F32).tobytes() and C.sizeof(abi.BodyShape) == 24 and C.sizeof(abi.BodyResult) == 8


# ------------------------------------------------------------------------------------------------ 3: order
@pytest.mark.parametrize("name", vc.SCENES)
def test_a_permuted_batch_gives_permuted_results(hook, references, name):
    n = len(references[name]["shaped"][0])
    order = [int(i) for i in np.random.default_rng(5).permutation(n)]
    assert order != list(range(n)) and order[0] != 0
    straight = run_batch(hook, references[name], "shaped", 1, ticks=4)
    permuted = run_batch(hook, references[name], "shaped", 1, ticks=4, order=order)
    for (sb, sr, si), (pb, pr, pi) in zip(straight, permuted):
        assert [sb[i] for i in order] == pb and [sr[i] for i in order] == pr and [si[i] for i in order] == pi


@pytest.mark.parametrize("name", vc.SCENES)
def test_a_body_alone_equals_the_body_in_the_batch(hook, references, name):
    """n = 1 for every body of the shapes batch against the same body in the whole batch; for the default shape also ycge_test_camera_tick_host"""
    ref = references[name]
    seqs, names, _ = ref["shaped"]
    whole = run_batch(hook, ref, "shaped", 1, ticks=4)
    w = abi.CameraWorld(*ref["world"])
    for i, (seq, shape) in enumerate(zip(seqs, names)):
        cb = vc.c_callback(ref["hit"])
        alone = bc.body_array([seq])
        single = vc.new_body(seq[0], seq[1])
        for k in range(4):
            _, dt_ms, run_update = seqs[0][2][k]
            rc, results, infos, msg = bc.tick_hook(hook, alone, bc.shape_array([shape]), w, [seq[2][k][0]], dt_ms, run_update, cb, 1)
            assert rc == abi.YCGE_OK and results == [(0, -1)], msg
            assert bytes(alone[0]) == whole[k][0][i] and infos[0] == whole[k][2][i], (i, shape, k)
            if shape == "default":
                rc, info, msg = vc.tick_hook(hook, single, w, seq[2][k][0], dt_ms, run_update, cb, 1)
                assert rc == abi.YCGE_OK and bytes(single) == whole[k][0][i] and info == whole[k][2][i], (i, k, msg)


# ------------------------------------------------------------------------------------------------ 4: one body in a corner
@ORDERS
def test_a_capped_body_does_not_cost_its_neighbours_their_tick(hook, windowed):
    """three bodies told apart by where their rays start: the middle one (x near 0) is in the corner of test_a_slide_that_never_ends_reaches_the_cap,
    the first (x near 100) in open air, the last (x near -100) over a floor at y = 0"""
    def scene(o, d, tmin, tmax):
        x = float(o[0])
        if x > 50.0:
            return None
        if x < -50.0:
            t = float(o[1])                                                     # straight down onto y = 0
            return (F32(t), (F32(0.0), F32(1.0), F32(0.0))) if d[1] < 0 and d[0] == 0 and d[2] == 0 and float(tmin) <= t <= float(tmax) else None
        if d[1] != 0: return None
        l = np.sqrt(float(d[0]) ** 2 + float(d[2]) ** 2)
        dx, dz = float(d[0]) / l, float(d[2]) / l
        s = np.sqrt(0.5)
        return F32(0.05), (F32(-(dx * s - dz * s)), F32(0.0), F32(-(dx * s + dz * s)))

    starts = [(100.0, 2.0, 0.0), (0.0, 2.0, 0.0), (-100.0, 1.9, 0.0)]
    moves = [[(vr.MOVE_HORIZONTAL, 0, 0.5, 0.25)], [(vr.MOVE_JUMP, 0, 0.0, 0.0), (vr.MOVE_HORIZONTAL, 0, 1.0, 0.0)], [(vr.MOVE_HORIZONTAL, 0, 0.0, 0.3), (vr.MOVE_JUMP, 0, 0.0, 0.0)]]
    w = abi.CameraWorld(*vc.WORLD_BOXES)
    bodies = (abi.CameraBody * 3)(*[vc.new_body(p, True) for p in starts])
    before = [bytes(b) for b in bodies]
    recs, first = bc.pack_moves(moves)
    results = (abi.BodyResult * 3)()
    info = (abi.CameraTickInfo * 3)()
    C.memset(info, 0xAB, C.sizeof(info))
    C.memset(results, 0xAB, C.sizeof(results))
    msg = C.create_string_buffer(256)
    rc = hook.ycge_test_bodies_tick_host(bodies, None, 3, C.byref(w), recs, first, 16.0, 1, results, info, vc.c_callback(scene), None, windowed, msg, 256)
    assert rc == abi.YCGE_OK, msg.value
    assert [(r.status, r.bad_move) for r in results] == [(0, -1), (1, 1), (0, -1)]
    assert bytes(bodies[1]) == before[1] and bytes(info[1]) == b"\xab" * 48
    for i in (0, 2):
        solo = vc.new_body(starts[i], True)
        rc, want, m = vc.tick_hook(hook, solo, w, moves[i], 16.0, True, vc.c_callback(scene), windowed)
        assert rc == abi.YCGE_OK, m
        assert bytes(bodies[i]) == bytes(solo) != before[i] and bc.info_dict(info[i]) == want


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_refusals_name_the_body_and_write_nothing(hook):
    miss = vc.c_callback(lambda o, d, tmin, tmax: None)
    nan, inf = float("nan"), float("inf")
    N = 4

    def call(n=N, bodies="ok", shapes=None, world="ok", moves="ok", first="ok", dt=16.0, results="ok", cb=miss, poke=None):
        """one call with everything good except what is named; poke(bodies, shapes, world, moves, first) edits the good arrays.  Returns
        (rc, message) and checks that nothing was written"""
        b = (abi.CameraBody * N)(*[vc.new_body((float(i), 2.0, 0.0), True) for i in range(N)])
        s = (abi.BodyShape * N)(*[abi.BodyShape(*abi.BODY_SHAPE_DEFAULT) for _ in range(N)]) if shapes == "ok" else None
        w = abi.CameraWorld(*vc.WORLD_BOXES)
        m, f = bc.pack_moves([[(vr.MOVE_HORIZONTAL, 0, 0.1, 0.0)], [], [(vr.MOVE_HORIZONTAL, 0, 0.1, 0.0), (vr.MOVE_VERTICAL, 0, 0.2, 0.0)], [(vr.MOVE_JUMP, 0, 0.0, 0.0)]])
        if poke: poke(b, s, w, m, f)
        r = (abi.BodyResult * N)()
        info = (abi.CameraTickInfo * N)()
        C.memset(r, 0xAB, C.sizeof(r)); C.memset(info, 0xAB, C.sizeof(info))
        snap = bytes(b)
        msg = C.create_string_buffer(256)
        rc = hook.ycge_test_bodies_tick_host(b if bodies == "ok" else None, s, n, C.byref(w) if world == "ok" else None, m if moves == "ok" else None,
                                             f if first == "ok" else None, dt, 1, r if results == "ok" else None, info, cb, None, 1, msg, 256)
        if rc != abi.YCGE_OK:
            assert bytes(b) == snap and bytes(r) == b"\xab" * C.sizeof(r) and bytes(info) == b"\xab" * C.sizeof(info)
        return rc, msg.value.decode()

    assert call()[0] == abi.YCGE_OK and call(shapes="ok")[0] == abi.YCGE_OK
    for n in (-1, abi.BODIES_MAX + 1):
        rc, msg = call(n=n)
        assert rc == abi.YCGE_ERR_INVALID_ARG and "YCGE_BODIES_MAX" in msg
    for null in ("bodies", "world", "results", "first"):
        rc, msg = call(**{null: None})
        assert rc == abi.YCGE_ERR_INVALID_ARG and "NULL" in msg, null
    rc, msg = call(moves=None)
    assert rc == abi.YCGE_ERR_INVALID_ARG and "body 0:" in msg and "NULL moves" in msg
    assert call(cb=C.cast(None, abi.CAMERA_HIT_FN))[0] == abi.YCGE_ERR_INVALID_ARG

    def poked(fn, want_rc=abi.YCGE_ERR_INVALID_ARG, **kw):
        rc, msg = call(poke=fn, **kw)
        assert rc == want_rc, msg
        return msg

    def set_first(*vals):
        def fn(b, s, w, m, f):
            f[:] = vals
        return fn
    assert "body 0:" in poked(set_first(1, 1, 3, 4, 4))                            # move_first[0] != 0
    assert "body 1:" in poked(set_first(0, 2, 1, 4, 4)) and "decreases" in poked(set_first(0, 2, 1, 4, 4))

    def too_many(b, s, w, m, f):
        f[:] = (0, 1, 1, 1 + abi.CAMERA_MAX_MOVES + 1, 1 + abi.CAMERA_MAX_MOVES + 1)
    msg = poked(too_many)                                                       # (refused before a move is read: the array is not that long)
    assert "body 2:" in msg and "YCGE_CAMERA_MAX_MOVES" in msg

    def body_field(field, v):
        def fn(b, s, w, m, f):
            if field in ("pos", "repel_vel"): getattr(b[2], field)[1] = v
            else: setattr(b[2], field, v)
        return fn
    for field, v in (("pos", nan), ("vertical_velocity", inf), ("shift_hold_timer", nan), ("repel_vel", -inf)):
        msg = poked(body_field(field, v))
        assert "body 2:" in msg and "finite" in msg and "move" not in msg.split("body 2:")[1], msg

    def move_of_body_2(kind, a, b_):
        def fn(b, s, w, m, f):
            m[2].kind, m[2].a, m[2].b = kind, a, b_                          # body 2's moves are m[1], m[2]: its own move 1
        return fn
    for (kind, a, b_), word in (((vr.MOVE_HORIZONTAL, 64.5, 0.0), "longer"), ((vr.MOVE_HORIZONTAL, 46.0, 46.0), "longer"), ((vr.MOVE_VERTICAL, -64.5, 0.0), "longer"),
                                ((4, 0.0, 0.0), "kind"), ((-1, 0.0, 0.0), "kind"), ((vr.MOVE_HORIZONTAL, nan, 0.0), "finite"), ((vr.MOVE_JUMP, 0.0, inf), "finite")):
        msg = poked(move_of_body_2(kind, a, b_))
        assert "body 2: move 1:" in msg and word in msg, msg

    def world_nan(b, s, w, m, f):
        w.water_level = nan
    assert "world" in poked(world_nan)
    for dt in (nan, inf, -inf):
        assert "delta_time_ms" in call(dt=dt)[1] and call(dt=dt)[0] == abi.YCGE_ERR_INVALID_ARG

    def shape_field(field, v):
        def fn(b, s, w, m, f):
            setattr(s[1], field, v)
        return fn
    bad_shapes = [(f, nan) for f, _ in abi.BodyShape._fields_] + [("jump_speed", inf), ("eye_height", 0.0), ("eye_height", -1.7), ("collision_radius", 0.0),
                                                                 ("collision_radius", -0.1), ("probe_radius", 0.0), ("gravity_accel", 0.0), ("gravity_accel", -9.81),
                                                                 ("ground_clearance", -0.01), ("jump_speed", -1.0), ("eye_height", 64.5), ("collision_radius", 64.5)]
    for field, v in bad_shapes:
        msg = poked(shape_field(field, v), shapes="ok")
        assert "body 1:" in msg and "shape" in msg, (field, v, msg)
    for field, v in (("eye_height", 64.0), ("collision_radius", 64.0), ("ground_clearance", 0.0), ("jump_speed", 0.0)):       # the limits themselves are accepted
        poked(shape_field(field, v), want_rc=abi.YCGE_OK, shapes="ok")
    # n = 0: nothing to do, nothing needed
    msg = C.create_string_buffer(64)
    assert hook.ycge_test_bodies_tick_host(None, None, 0, None, None, None, 16.0, 1, None, None, miss, None, 1, msg, 64) == abi.YCGE_OK
