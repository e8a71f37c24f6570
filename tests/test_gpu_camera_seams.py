"""-m gpu: the camera tick and the bodies tick (k_camera_tick, k_bodies_tick in csrc/ycge_camera.hip) on the seams of the physics
(tests/camera_seams.py: bodies on and within an ulp of the stepper's thresholds, walls exactly at a ray's tMax, ties, the lattice), against
the restatement (tests/volume_camera_restatement.py) over the oracle's Scene.Hit - body words, rays_committed and every event counter equal
after every tick, bit for bit, on both kernel instances (analytic boxes without a grid, a voxel world).  That the cases reach their seams
is held without a GPU (tests/test_camera_seams_cpu.py).  No test here reaches a cap or a non-finite position: status 1..3 rests on the
stepper shared with the hook."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_seams as cs
import volume_camera_cases as vc
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import flatten

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def references(oracle):
    """per scene: {case: the restatement's (body words, counters) after every tick over the oracle} - computed once"""
    out = {}
    for name in cs.SCENES:
        sc = cs.scene(name)
        o = oracle.OracleRenderer(sc, 16, 8, 1, None, flat=flatten(sc))
        hit = vc.oracle_hit(o)
        out[name] = {c: cs.restate(c, hit)[0] for c in cs.cases(name)}
        o.close()
    return out


def solo_ticks(g, c):
    """the case through ycge_volume_camera_tick: [(body bytes, info)] after every tick"""
    b, w = c.body(), abi.CameraWorld(*c.world)
    rows = []
    for moves, dt_ms, run_update in c.ticks:
        info = g.CameraTick(b, w, moves, dt_ms, run_update)
        rows.append((bytes(b), info))
    return rows


def check_windows(info, what):
    assert info["rays_walked"] >= info["rays_committed"] >= info["windows"], (what, info)


# ------------------------------------------------------------------------------------------------ 1: the single tick
@pytest.mark.parametrize("name", cs.SCENES)
def test_single_tick_matches_the_restatement(product_lib, references, name):
    """ycge_volume_camera_tick on every default-shape case; in the wedged push-out case rays behind a moved body were dropped"""
    g = RaytraceRenderer(flatten(cs.scene(name)), 32, 16, 45.0, 1)
    try:
        n = 0
        for c in cs.cases(name, shape="default"):
            want = references[name][c]
            for k, (raw, info) in enumerate(solo_ticks(g, c)):
                b = abi.CameraBody.from_buffer_copy(raw)
                vc.assert_same(b, info, want[k][0], want[k][1], (c, k))
                check_windows(info, (c, k))
                if c.cls == "push" and c.name == "wedged":
                    assert info["rays_walked"] > info["rays_committed"], (c, info)
            n += 1
        assert n >= 100
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ 2: the bodies tick
def run_batch(g, group, want, solo):
    """the cases of one batch through ycge_volume_bodies_tick, each with its own shape, held to the restatement after every tick and -
    where the shape is the reference's - to the solo tick"""
    bodies = (abi.CameraBody * len(group))(*[c.body() for c in group])
    shapes = (abi.BodyShape * len(group))(*[cs.shape_struct(c.shape) for c in group])
    w = abi.CameraWorld(*group[0].world)
    for k, (_, dt_ms, run_update) in enumerate(group[0].ticks):
        results, infos = g.BodiesTick(bodies, w, [c.ticks[k][0] for c in group], dt_ms, run_update, shapes)
        assert results == [(0, -1)] * len(group), (group[0], k, results)
        for i, c in enumerate(group):
            vc.assert_same(bodies[i], infos[i], want[c][k][0], want[c][k][1], (c, k, len(group), i))
            check_windows(infos[i], (c, k))
            if c.cls == "push" and c.name == "wedged":
                assert infos[i]["rays_walked"] > infos[i]["rays_committed"], (c, infos[i])
            if c in solo:
                assert bytes(bodies[i]) == solo[c][k][0] and infos[i] == solo[c][k][1], (c, k, "solo")


@pytest.mark.parametrize("name", cs.SCENES)
def test_bodies_tick_matches_the_restatement_in_any_order(product_lib, references, name):
    """all cases of the scene, one batch per world and (dt, run_update): in case order, in a fixed permuted order - a body's result does not
    depend on its workgroup - and one case of every class as a batch of n = 1"""
    want = references[name]
    g = RaytraceRenderer(flatten(cs.scene(name)), 32, 16, 45.0, 1)
    try:
        solo = {c: solo_ticks(g, c) for c in cs.cases(name, shape="default")}
        rng = np.random.default_rng(5)
        for group in cs.batches(name):
            assert len(group) <= abi.BODIES_MAX
            run_batch(g, group, want, solo)
            if len(group) > 1:
                run_batch(g, [group[i] for i in rng.permutation(len(group))], want, solo)
        for cls in cs.CLASSES:
            picked = cs.cases(name, cls)
            run_batch(g, [picked[len(picked) // 2]], want, solo)
            run_batch(g, [picked[-1]], want, solo)
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ 3: YCGE_CAMERA_HOST=1 in a fresh process
def test_host_route_matches_the_restatement(product_lib, references):
    """the single tick with the stepper on the host, a window a batch of scene queries: a child process made with YCGE_CAMERA_HOST=1"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(cs.__file__)))
    path = os.pathsep.join([root, os.path.join(root, "tests")] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else []))
    env = dict(os.environ, YCGE_CAMERA_HOST="1", PYTHONPATH=path)
    r = subprocess.run([sys.executable, cs.__file__, "--run-cases"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for name in cs.SCENES:
        mine = cs.cases(name, shape="default")
        assert len(got[name]) == len(mine)
        for c, rows in zip(mine, got[name]):
            want = references[name][c]
            assert len(rows) == len(want)
            for k, (words, info) in enumerate(rows):
                assert np.array_equal(np.array(words, np.uint32), want[k][0]), (c, k)
                for key in ("rays_committed",) + vc.EVENTS:
                    assert info[key] == want[k][1][key], (c, k, key)
                check_windows(info, (c, k))
