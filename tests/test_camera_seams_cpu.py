"""The seams of the camera physics without a GPU (tests/camera_seams.py): first the conditions of the inputs themselves, on the restatement
(tests/volume_camera_restatement.py) over the oracle's Scene.Hit alone - every class reaches the comparisons it was built for, with both
sides equal or within its fan, and both outcomes occur; a class that never reaches its seam fails here - then the library's stepper
(csrc/ycge_camera_physics.h through ycge_test_camera_tick_host and ycge_test_bodies_tick_host, serial and windowed) held to the
restatement on every case: the body bit for bit, rays_committed and every event counter equal, status 0.

No device is touched: the hooks take Scene.Hit as a C callback."""
import numpy as np
import pytest

import camera_seams as cs
import volume_bodies_cases as bc
import volume_camera_cases as vc
import volume_camera_restatement as vr
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.scene import flatten

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def runs(oracle):
    """per scene: the oracle's Scene.Hit and, per case, the restatement's (rows, most micro-steps of a move, observer log) - computed once"""
    out, keep = {}, []
    for name in cs.SCENES:
        sc = cs.scene(name)
        o = oracle.OracleRenderer(sc, 16, 8, 1, None, flat=flatten(sc))
        keep.append(o)
        hit = vc.oracle_hit(o)
        per_case = {}
        for c in cs.cases(name):
            log = []
            rows, max_micro = cs.restate(c, hit, log)
            per_case[c] = (rows, max_micro, log)
        out[name] = (hit, per_case)
    yield out
    for o in keep:
        o.close()


@pytest.fixture(scope="module")
def hook(product_lib):
    assert hasattr(product_lib, "ycge_test_camera_tick_host") and hasattr(product_lib, "ycge_test_bodies_tick_host")
    return vc.bind_hook(product_lib)


# ------------------------------------------------------------------------------------------------ 1: the inputs
def test_the_cases_are_what_the_module_says():
    assert 300 <= len(cs.CASES) <= 900
    for c in cs.CASES:
        assert c.cls in cs.CLASSES and c.scene in cs.SCENES and c.shape in cs.SHAPES and 1 <= len(c.ticks) <= 3
        for moves, dt_ms, _ in c.ticks:
            assert len(moves) <= abi.CAMERA_MAX_MOVES and -100.0 <= dt_ms <= 200.0
    for name in cs.SCENES:
        assert {c.cls for c in cs.cases(name)} == set(cs.CLASSES)
        assert sum(len(b) for b in cs.batches(name)) == len(cs.cases(name))
    lattice = np.array([v for lo, hi in cs.BOXES for v in lo + hi], F64) * 16.0
    assert np.array_equal(lattice, np.round(lattice)) and np.abs(lattice).max() < 64 * 16
    for g in cs.scene("voxels").Objects:
        corner = np.array(g.MinCorner, F64) * 16.0
        assert np.array_equal(corner, np.round(corner)) and tuple(g.VoxelSize) == (1.0, 1.0, 1.0)
    assert cs.SHAPES["low"][0] + cs.SHAPES["low"][3] <= 1.0 and cs.SHAPES["wide"][1] == 2.0


def test_no_case_comes_near_the_cap(runs):
    """none is left out: the restatement takes at most CAMERA_MAX_MICRO_STEPS // 4 micro-steps for any move of any case"""
    for name in cs.SCENES:
        for c, (_, max_micro, _) in runs[name][1].items():
            assert max_micro <= abi.CAMERA_MAX_MICRO_STEPS // 4, (c, max_micro)


def _table_row(name, cls, seam, entries):
    near, exact, outcomes, differ = cs.seam_report(entries, *seam)
    return f"{cls:15s} {name:7s} {seam[0]:15s} cases {len(entries):3d}  within the fan {len(near):3d}  exactly {len(exact):3d}  outcomes {sorted(outcomes)}"


@pytest.mark.parametrize("cls", cs.CLASSES)
@pytest.mark.parametrize("name", cs.SCENES)
def test_class_reaches_its_seams(runs, name, cls):
    """for every seam of the class that exists in the scene: some case brings the comparison's two sides together (bit-equal where SEAMS
    says 0), and the fans that do show both outcomes - for rec.T against tMax, both a hit and a miss of such a ray"""
    entries = [(c, log) for c, (_, _, log) in runs[name][1].items() if c.cls == cls]
    assert len(entries) >= 3
    for seam in cs.SEAMS[cls]:
        comparison, tol, where = seam
        if name not in where:
            continue
        near, exact, outcomes, differ = cs.seam_report(entries, comparison, tol)
        print(_table_row(name, cls, (comparison, tol), entries))
        assert near, (cls, name, comparison, "never reached")
        if tol == 0:
            assert exact, (cls, name, comparison, "never with both sides equal")
        if comparison.startswith("hit:"):
            assert differ, (cls, name, comparison, "no fan in which such a ray both hits and misses")
        else:
            assert outcomes == {True, False}, (cls, name, comparison, outcomes)


@pytest.mark.parametrize("cls, group, scenes", [("capsule_tie", "hit:caps", ("boxes",)), ("exit_tie", "hit:exit", cs.SCENES), ("embed", "hit:embed", cs.SCENES)])
def test_tie_classes_have_rays_of_bit_equal_t(runs, cls, group, scenes):
    """two rays of one group of one case hit at the same binary32 t (capsule: behind the first, so both reached `cand < best`)"""
    for name in scenes:
        tied = 0
        for c, (_, _, log) in runs[name][1].items():
            if c.cls != cls: continue
            ts = [F32(left).view(np.uint32) for n, left, _, outcome in log if n == group and outcome]
            tied += len(ts) != len(set(int(t) for t in ts))
        assert tied >= 2, (cls, name, tied)


def test_move_cutoff_has_sums_that_round_across(runs):
    """some (a, b) of the `round` family are ignored although their exact length is above 1e-6, others of it are taken: the sum of squares
    is a binary32 sum"""
    for name in cs.SCENES:
        across = taken = 0
        for c, (rows, _, log) in runs[name][1].items():
            if c.cls != "move_cutoff" or c.family != "round": continue
            (_, _, a, b), _ = c.ticks[0][0]
            exact_len = np.sqrt(F64(F32(a)) * F64(F32(a)) + F64(F32(b)) * F64(F32(b)))
            ignored = [o for n, _, _, o in log if n == "h_cutoff"]
            assert len(ignored) == 2 and ignored[0] == ignored[1], c
            across += bool(ignored[0] and exact_len > 1e-6)
            taken += not ignored[0]
            assert rows[0][1]["micro_steps"] == (0 if ignored[0] else 2), c
        assert across >= 3 and taken >= 2, (name, across, taken)


def test_the_wedged_bodies_are_moved_ray_after_ray(runs):
    for name in cs.SCENES:
        wedged = [rows[-1][1]["push_outs"] for c, (rows, _, _) in runs[name][1].items() if c.cls == "push" and c.name == "wedged"]
        assert wedged and max(wedged) >= 6, (name, wedged)


def test_events_of_the_classes(runs):
    """what the cases are for happens somewhere: every event counter, 32 moves, a move of 92 micro-steps or more"""
    for name in cs.SCENES:
        total = dict.fromkeys(vc.EVENTS, 0)
        most = 0
        for c, (rows, max_micro, _) in runs[name][1].items():
            for _, counters in rows:
                for k in total: total[k] += counters[k]
            most = max(most, max_micro)
        assert all(v > 0 for v in total.values()), (name, total)
        assert most >= 92, (name, most)                            # (the move of length 64 with a micro-step of 0.7)
        assert any(len(m) == abi.CAMERA_MAX_MOVES for c in cs.cases(name, "limits") for m, _, _ in c.ticks)


# ------------------------------------------------------------------------------------------------ 2: the observer changes nothing
def test_the_observer_changes_nothing(runs):
    for name in cs.SCENES:
        hit, per_case = runs[name]
        for c, (rows, max_micro, log) in per_case.items():
            plain, plain_micro = cs.restate(c, hit)
            assert plain_micro == max_micro and len(plain) == len(rows) and log
            for (w0, c0), (w1, c1) in zip(plain, rows):
                assert np.array_equal(w0, w1) and c0 == c1, c


def test_dmax_dmin_treat_zeros_as_math_max_and_min():
    """Math.Max(+0, -0) is +0 and Math.Min is -0, whatever the order; a NaN wins (the stepper's dmax / dmin do the same)"""
    pz, nz, nan = F64(0.0), F64(-0.0), F64(np.nan)
    for a, b in ((pz, nz), (nz, pz)):
        assert not np.signbit(vr.dmax(a, b)) and np.signbit(vr.dmin(a, b))
    assert np.signbit(vr.dmax(nz, nz)) and not np.signbit(vr.dmin(pz, pz))
    assert vr.dmax(1.0, 2.0) == 2.0 and vr.dmin(1.0, 2.0) == 1.0 and vr.dmax(-1.0, nz) == 0.0 and np.signbit(vr.dmax(-1.0, nz))
    assert np.isnan(vr.dmax(nan, 1.0)) and np.isnan(vr.dmax(1.0, nan)) and np.isnan(vr.dmin(nan, 1.0)) and np.isnan(vr.dmin(1.0, nan))


# ------------------------------------------------------------------------------------------------ 3: the stepper's host compilation
@pytest.mark.parametrize("windowed", [0, 1], ids=["serial", "windowed"])
@pytest.mark.parametrize("name", cs.SCENES)
def test_camera_hook_matches_the_restatement(hook, runs, name, windowed):
    """ycge_test_camera_tick_host (the reference's shape) on every default-shape case, tick by tick"""
    hit, per_case = runs[name]
    cb = vc.c_callback(hit)
    n = 0
    for c, (rows, _, _) in per_case.items():
        if c.shape != "default": continue
        b, w = c.body(), abi.CameraWorld(*c.world)
        for k, (moves, dt_ms, run_update) in enumerate(c.ticks):
            rc, info, msg = vc.tick_hook(hook, b, w, moves, dt_ms, run_update, cb, windowed)
            assert rc == abi.YCGE_OK, (c, k, msg)
            vc.assert_same(b, info, rows[k][0], rows[k][1], (c, k))
            assert info["rays_walked"] >= info["rays_committed"] >= info["windows"] or not windowed
            if not windowed:
                assert info["rays_walked"] == info["rays_committed"] == info["windows"]
        n += 1
    assert n >= 100 and cb.py.calls > 0


@pytest.mark.parametrize("windowed", [0, 1], ids=["serial", "windowed"])
@pytest.mark.parametrize("name", cs.SCENES)
def test_bodies_hook_matches_the_restatement(hook, runs, name, windowed):
    """ycge_test_bodies_tick_host on every case, each with its own shape: one batch per world and clock"""
    hit, per_case = runs[name]
    cb = vc.c_callback(hit)
    walked = committed = 0
    for group in cs.batches(name):
        bodies = (abi.CameraBody * len(group))(*[c.body() for c in group])
        shapes = (abi.BodyShape * len(group))(*[cs.shape_struct(c.shape) for c in group])
        w = abi.CameraWorld(*group[0].world)
        for k, (_, dt_ms, run_update) in enumerate(group[0].ticks):
            rc, results, infos, msg = bc.tick_hook(hook, bodies, shapes, w, [c.ticks[k][0] for c in group], dt_ms, run_update, cb, windowed)
            assert rc == abi.YCGE_OK, (group[0], k, msg)
            for i, c in enumerate(group):
                assert results[i] == (0, -1), (c, k, results[i])
                rows = per_case[c][0]
                vc.assert_same(bodies[i], infos[i], rows[k][0], rows[k][1], (c, k))
                if windowed:
                    assert infos[i]["rays_walked"] >= infos[i]["rays_committed"] >= infos[i]["windows"], (c, k)
                else:
                    assert infos[i]["rays_walked"] == infos[i]["rays_committed"] == infos[i]["windows"], (c, k)
                walked += infos[i]["rays_walked"]; committed += infos[i]["rays_committed"]
    assert walked > committed if windowed else walked == committed
