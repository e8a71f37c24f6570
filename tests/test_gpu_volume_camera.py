"""-m gpu: VolumeScene's camera physics on the device, one launch a tick (ycge_volume_camera_tick, csrc/ycge_camera.*), against the
restatement (tests/volume_camera_restatement.py) over the oracle's Scene.Hit - the body after every tick bit for bit, rays_committed and
every event counter equal - on the drawn sequences of tests/volume_camera_cases.py and both kernel instances (a voxel world, analytic
boxes without a grid)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_util as pu
import volume_camera_cases as vc
import volume_camera_restatement as vr
from yetanotherconsolegameengine_amd import abi, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer, VolumeCamera
from yetanotherconsolegameengine_amd.scene import AmbientLight, Scene, VolumeGrid, flatten, vec3

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def references(oracle):
    """per scene: the world, the drawn sequences and the restatement's result after every tick over the oracle - computed once"""
    out = {}
    for name in vc.SCENES:
        sc, world, starts = vc.make_scene(name)
        o = oracle.OracleRenderer(sc, 16, 8, 1, None, flat=flatten(sc))
        seqs = {seed: vc.draw_sequence(seed, starts) for seed in vc.SEEDS[name]}
        refs = {seed: vc.run_restatement(vc.oracle_hit(o), world, seq)[0] for seed, seq in seqs.items()}
        o.close()
        out[name] = (sc, world, seqs, refs)
    return out


def moves_of(rows):
    return [abi.CameraMove(int(k), int(s), float(a), float(b)) for k, s, a, b in rows]


# ------------------------------------------------------------------------------------------------ 1: the kernel against the restatement
@pytest.mark.parametrize("name", vc.SCENES)
def test_device_ticks_match_the_restatement(product_lib, references, name):
    sc, world, seqs, refs = references[name]
    g = RaytraceRenderer(flatten(sc), 32, 16, 45.0, 1)
    try:
        w = abi.CameraWorld(*world)
        walked = committed = 0
        for seed, (start, auto_placed, ticks) in seqs.items():
            b = vc.new_body(start, auto_placed)
            for i, (moves, dt_ms, run_update) in enumerate(ticks):
                info = g.CameraTick(b, w, moves_of(moves), dt_ms, run_update)
                vc.assert_same(b, info, refs[seed][i][0], refs[seed][i][1], (name, seed, i))
                assert info["rays_walked"] >= info["rays_committed"] >= info["windows"]
                walked += info["rays_walked"]; committed += info["rays_committed"]
        assert walked > committed
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ 2: YCGE_CAMERA_HOST=1 in a fresh process
def test_host_route_matches_the_restatement(product_lib, references):
    """the same sequences with the stepper on the host, a window a batch of scene queries: a child process made with YCGE_CAMERA_HOST=1"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(vc.__file__)))
    path = os.pathsep.join([root, os.path.join(root, "tests")] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else []))
    env = dict(os.environ, YCGE_CAMERA_HOST="1", PYTHONPATH=path)
    r = subprocess.run([sys.executable, vc.__file__, "--run-sequences"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for name in vc.SCENES:
        _, _, seqs, refs = references[name]
        for seed in seqs:
            rows = got[name][str(seed)]
            assert len(rows) == len(refs[seed])
            for i, (words, info) in enumerate(rows):
                want, counters = refs[seed][i]
                assert np.array_equal(np.array(words, np.uint32), want), (name, seed, i)
                for k in ("rays_committed",) + vc.EVENTS:
                    assert info[k] == counters[k], (name, seed, i, k)


# ------------------------------------------------------------------------------------------------ 3: speculation is real
def test_windows_of_a_quiet_tick(product_lib):
    """open air, no moves: the embed test's 8 rays are one window, each ground fan one, and a push-out call whose rays all miss is one
    (both passes share it) - at most 5 by the order of Update, 4 as built; with the fly timer running there are no fans: at most 3"""
    g = RaytraceRenderer(flatten(vc.box_scene()), 32, 16, 45.0, 1)
    try:
        w = abi.CameraWorld(*vc.WORLD_BOXES)
        b = vc.new_body((0.0, 60.0, 0.0), True)
        info = g.CameraTick(b, w, [], 16.0, True)
        assert info["windows"] <= 5 and info["rays_committed"] == 8 + 5 + 5 + 32 and info["rays_walked"] == info["rays_committed"]
        b = vc.new_body((0.0, 60.0, 0.0), True)
        info = g.CameraTick(b, w, moves_of([(vr.MOVE_SHIFT, 0, 0.0, 0.0)]), 16.0, True)
        assert info["windows"] <= 3 and info["rays_committed"] == 8 + 32
        assert b.pos[1] == 60.0 and b.vertical_velocity == 0.0
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ 4: attaches, edits and ticks interleaved
def _slab(cells, corner):
    return VolumeGrid(np.ascontiguousarray(cells), vec3(*corner), vec3(1, 1, 1), scenes.VoxelMaterialLookup)


def _volume_scene(grids):
    s = Scene()
    s.IsVolumeScene = True
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.2)
    s.Objects = list(grids)
    return s


def test_ticks_between_attaches_and_edits(product_lib, oracle):
    """a floor chunk, then a wall chunk attached beside it, then cells dug under the body and cells placed in its way: each tick sees the scene
    of the last change - the body walks into the attached wall, falls into the dug pit on the next tick, is blocked by the placed cells -
    and equals the restatement over an oracle of the equivalent scene"""
    floor = np.zeros((8, 6, 8, 2), np.int32); floor[:, :3, :, 0] = scenes.STONE            # x, z in [-4, 4), top at y = 3
    wall = np.zeros((2, 6, 8, 2), np.int32); wall[:, :, :, 0] = scenes.STONE               # x in [4, 6)
    A = _slab(floor, (-4, 0, -4))
    B = _slab(wall, (4, 0, -4))
    scene = _volume_scene([A])
    g = RaytraceRenderer(flatten(scene), 32, 16, 45.0, 1)
    world = (6.0, 1.0, 1.0)
    w = abi.CameraWorld(*world)
    b = vc.new_body((0.5, 3.0 + 1.8, 0.5), True)
    cam = vr.VolumeCamera(None, (0.5, 3.0 + 1.8, 0.5), *world, auto_placed=True)
    oracles = []

    def equivalent(grids):
        sc = _volume_scene(grids)
        o = oracle.OracleRenderer(sc, 16, 8, 1, None, flat=flatten(sc))
        oracles.append(o)
        cam.hit = vc.oracle_hit(o)

    def tick(moves, dt_ms, what):
        info = g.CameraTick(b, w, moves_of(moves), dt_ms, True)
        counters = cam.tick(moves, dt_ms, True)
        vc.assert_same(b, info, vc.restatement_words(cam), counters, what)
        return info

    try:
        equivalent([A])
        for k in range(2):
            tick([], 16.0, f"on the floor {k}")
        assert b.is_grounded and abs(b.pos[1] - 4.8) < 1e-5
        # the wall chunk arrives: a walk of 5 along +x ends in front of its face at x = 4
        scene.Objects = [A, B]
        g.StreamObjects(scene)
        equivalent([A, B])
        info = tick([(vr.MOVE_HORIZONTAL, 0, 5.0, 0.0)], 16.0, "into the attached wall")
        assert info["blocked_steps"] == 1 and info["push_outs"] >= 1 and 3.0 < b.pos[0] < 4.0
        # the cells under the body (and under its fan of +-0.35) are dug: it falls on the next tick and lands one cell lower
        ix = int(np.floor(b.pos[0] + 4.0))
        lo, hi = (ix - 1, 2, 3), (min(ix + 1, 7), 2, 5)
        g.EditVoxels([(g.flat._grid_index[id(A)], lo, hi, 0, 0)])
        dug = floor.copy(); dug[lo[0]:hi[0] + 1, 2, lo[2]:hi[2] + 1] = 0
        equivalent([_slab(dug, (-4, 0, -4)), B])
        y0 = b.pos[1]
        tick([], 100.0, "falling 0")
        assert b.pos[1] < y0 and not b.is_grounded
        for k in range(1, 8):
            tick([], 100.0, f"falling {k}")
        assert b.is_grounded and abs(b.pos[1] - 3.8) < 1e-5
        # two cells placed at the pit's far side, eye and torso high: the walk back along -x stops at them
        px = lo[0]
        g.EditVoxels([(g.flat._grid_index[id(A)], (px, 2, 3), (px, 4, 5), scenes.STONE, 0)])
        placed = dug.copy(); placed[px, 2:5, 3:6, 0] = scenes.STONE
        equivalent([_slab(placed, (-4, 0, -4)), B])
        info = tick([(vr.MOVE_HORIZONTAL, 0, -3.0, 0.0)], 16.0, "against the placed cells")
        assert info["blocked_steps"] == 1 and info["push_outs"] >= 1 and b.pos[0] > float(px - 4 + 1)          # (still on this side of them)
    finally:
        g.close()
        for o in oracles:
            o.close()


# ------------------------------------------------------------------------------------------------ 5: frames unaffected
POSES = [((0.0, 1.0, 0.0), 0.0, 0.0), ((0.0, 1.0, 0.0), 0.0, 0.0), ((0.05, 1.0, 0.1), 0.02, -0.01), ((0.05, 1.0, 0.1), 0.02, -0.01)]


def _player(g, cam, k):
    cam.forward(0.3 * k, 0.016)
    if k % 2: cam.jump()
    cam.tick(g, 16.0)


def test_frames_unaffected_synchronous(product_lib):
    """the same frames, bit for bit - SDR, TAA history, RNG state - with ticks between them and without"""
    sc, w, h, ss, pose = scenes.config_scene(2)
    flat = flatten(sc)
    out = []
    for with_ticks in (False, True):
        g = RaytraceRenderer(flat, 160, 45, 45.0, 1, capture_debug=True)
        cam = VolumeCamera((0.0, 3.0, 0.0), 16.0, 4.0, auto_placed=True)
        frames = []
        for k, (p, y, pt) in enumerate(POSES):
            g.SetCamera(p, y, pt)
            if with_ticks: _player(g, cam, k)
            sdr = g.TryFlipAndBlit(want_sdr=True)
            if with_ticks: _player(g, cam, 10 + k)
            frames.append((sdr, g.read(abi.BUF_TAA_HISTORY), g.read(abi.BUF_RNG_STATE), int(g.stats.frame)))
        out.append(frames)
        g.close()
    for a, b in zip(*out):
        assert pu.mismatch_count(a[0], b[0]) == 0 and pu.mismatch_count(a[1], b[1]) == 0 and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_frames_unaffected_in_flight(product_lib):
    """frames in flight: a tick between two of them does not join the one in flight - frames_outstanding stays 1 - and the frames are the
    ones the same sequence without ticks gives"""
    sc, w, h, ss, pose = scenes.config_scene(5, small=True, t01=0.5)
    flat = flatten(sc)
    p0 = pose["pos"]
    out = []
    for with_ticks in (False, True):
        g = RaytraceRenderer(flat, 160, 45, pose.get("fov", 45.0), 1)
        cam = VolumeCamera(p0, *vc.WORLD5, auto_placed=True)
        sdrs = []
        for k in range(4):
            g.SetCamera((p0[0] + 0.01 * k, p0[1], p0[2]), pose["yaw"], pose["pitch"])
            a = g.RenderAsync(sdr_slot=k % 2)
            if with_ticks:
                _player(g, cam, k)
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
    g0 = RaytraceRenderer(None, 16, 8, 45.0, 1)
    try:
        b = vc.new_body((0.0, 2.0, 0.0), True)
        before = bytes(b)
        with pytest.raises(abi.YcgeError) as e:
            g0.CameraTick(b, w, [], 16.0)
        assert e.value.status == abi.YCGE_ERR_NO_SCENE and bytes(b) == before
    finally:
        g0.close()
    sc = vc.box_scene()
    o = oracle.OracleRenderer(sc, 16, 8, 1, None, flat=flatten(sc))
    g = RaytraceRenderer(flatten(sc), 32, 16, 45.0, 1, devices=[0, 0])
    try:
        b = vc.new_body((0.0, 2.0, 0.0), True)
        before = bytes(b)
        good = (abi.CameraMove * 2)(abi.CameraMove(0, 0, 0.1, 0.0), abi.CameraMove(0, 0, 0.1, 0.0))
        info = abi.CameraTickInfo()
        call = lambda ctx, body, world, moves, n, dt=16.0: L.ycge_volume_camera_tick(ctx, body, world, moves, n, dt, 1, C.byref(info))
        assert call(None, C.byref(b), C.byref(w), good, 2) == abi.YCGE_ERR_INVALID_ARG
        peer = C.c_void_p(L.ycge_debug_peer_context(g.ctx, 0))
        assert peer.value
        assert call(peer, C.byref(b), C.byref(w), good, 2) == abi.YCGE_ERR_INVALID_ARG and b"driven by their root" in L.ycge_last_error(peer)
        for args in ((None, C.byref(w), good, 2), (C.byref(b), None, good, 2), (C.byref(b), C.byref(w), good, -1),
                     (C.byref(b), C.byref(w), good, abi.CAMERA_MAX_MOVES + 1), (C.byref(b), C.byref(w), None, 1),
                     (C.byref(b), C.byref(w), good, 2, float("nan"))):
            assert call(g.ctx, *args) == abi.YCGE_ERR_INVALID_ARG, args[2:]
            assert L.ycge_last_error(g.ctx).startswith(b"ycge_volume_camera_tick: ")
        for m, word in ((abi.CameraMove(0, 0, 65.0, 0.0), b"longer"), (abi.CameraMove(1, 0, -65.0, 0.0), b"longer"), (abi.CameraMove(7, 0, 0.0, 0.0), b"kind"),
                        (abi.CameraMove(0, 0, float("inf"), 0.0), b"finite")):
            bad = (abi.CameraMove * 2)(good[0], m)
            assert call(g.ctx, C.byref(b), C.byref(w), bad, 2) == abi.YCGE_ERR_INVALID_ARG
            msg = L.ycge_last_error(g.ctx)
            assert b"move 1:" in msg and word in msg, msg
        nb = vc.new_body((0.0, float("nan"), 0.0), True)
        snap = bytes(nb)
        assert call(g.ctx, C.byref(nb), C.byref(w), good, 2) == abi.YCGE_ERR_INVALID_ARG and bytes(nb) == snap
        assert bytes(b) == before and all(getattr(info, n) == 0 for n, _ in abi.CameraTickInfo._fields_)
        # and the context is usable and right afterwards (the root of a two-device context answers, as for the queries)
        cam = vr.VolumeCamera(vc.oracle_hit(o), (0.0, 2.0, 0.0), *vc.WORLD_BOXES, auto_placed=True)
        rows = [(vr.MOVE_HORIZONTAL, 0, 0.1, 0.0), (vr.MOVE_HORIZONTAL, 0, 0.1, 0.0)]
        got = g.CameraTick(b, w, moves_of(rows), 16.0)
        counters = cam.tick(rows, 16.0)
        vc.assert_same(b, got, vc.restatement_words(cam), counters, "after the refusals")
        g.TryFlipAndBlit()
    finally:
        o.close(); g.close()
