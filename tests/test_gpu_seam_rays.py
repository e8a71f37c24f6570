"""-m gpu: the scene walk (csrc/ycge_rt.hip.h) held to the oracle on rays aimed at its seams (tests/seam_rays.py; their conditions are held on
the CPU by test_seam_rays_cpu.py): origins in the planes of boxes with a zero direction component - the only rays on which box_scene's two
forms, and walk_phase against tree_phase, can differ -, rays through shared edges, vertices and rims, intervals that end on the hit to the
ulp, denominators on either side of their cut-offs, voxel walks along cell faces, edges and corners.

Scene.Hit and Scene.Occluded against orc_scene_hit, bit for bit - the hit flag, the object, the sub id (box face, cylinder part, triangle,
voxel cell), t, P, N, albedo - in every walk form a query can take, each class alone and all of them dealt into one batch; then whole frames
from camera positions exactly on seams, through the frame kernels the query does not instantiate."""
import numpy as np
import pytest

import parity_util as pu
import seam_rays as sr
from test_gpu_scene_queries import assert_records_equal, query_and_compare
from test_gpu_timed_variants import _check_walk_tree
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import flatten

pytestmark = pytest.mark.gpu

F32 = np.float32
KNOBS = ("YCGE_PATH", "YCGE_GENERIC_WALK", "YCGE_NO_ANALYTIC_WALK", "YCGE_NO_WALK_TREE")
# the walk forms a query can take: (id, the knob that selects it, the scenes it differs on)
FORMS = [("default", None, sr.SCENES), ("generic_walk", "YCGE_GENERIC_WALK", sr.SCENES), ("no_analytic_walk", "YCGE_NO_ANALYTIC_WALK", ("analytic",)),
         ("no_walk_tree", "YCGE_NO_WALK_TREE", ("voxels",))]
POSE = dict(pos=(0.0, 1.0, 0.0), yaw=0.0, pitch=0.0, fov=45.0)


@pytest.fixture(scope="module")
def seams(oracle):
    """per scene: the flat scene, the oracle's renderer, and per class (rays, labels, flag, records) - the reference, computed once, shared by
    every form and left unchanged"""
    out = {}
    for name in sr.SCENES:
        flat = flatten(sr.scene(name))
        o = oracle.OracleRenderer(sr.scene(name), 48, 16, 1, POSE, flat=flat)
        cls = {}
        for c in sr.CLASSES:
            rays, labels = sr.class_rays(name, c, o)
            flag, rec = sr.oracle_records(o, rays)
            for a in (rays, flag, rec): a.setflags(write=False)
            cls[c] = (rays, labels, flag, rec)
        out[name] = (flat, o, cls)
    yield out
    for _, o, _ in out.values():
        o.close()


def _set_form(monkeypatch, knob):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if knob:
        monkeypatch.setenv(knob, "1")


def _compare(g, rays, flag, rec, what):
    hits, ids = g.Hit(rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7])
    occl = g.Occluded(rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7])
    assert_records_equal(rays, hits, ids, occl, flag, rec, what)


@pytest.mark.parametrize("name,form,knob", [(n, f, k) for f, k, names in FORMS for n in names], ids=[f"{n}-{f}" for f, _, names in FORMS for n in names])
def test_queries_on_seam_rays(product_lib, seams, monkeypatch, name, form, knob):
    """every class alone, then all classes dealt round-robin into one batch: a wavefront then holds lanes with three finite reciprocals
    (walk_phase, box_scene's plain form) beside lanes without, and parked lanes beside walking ones.  Every form gives the oracle's records."""
    _set_form(monkeypatch, knob)
    flat, o, cls = seams[name]
    g = RaytraceRenderer(flat, 48, 16, POSE["fov"], 1)
    try:
        # the form is the one the case is named for.  A walk tree exists exactly where a scene with a grid object is walked without
        # YCGE_NO_WALK_TREE (read back from the device and checked node by node); `analytic` alone has neither mesh nor grid, which is all SceneDev::analytic_only asks (test_seam_rays_cpu.py holds that
        # of the scenes; the flag itself has no read-back, and the issue rules out new hooks)
        walk_nodes = _check_walk_tree(g, sr.scene(name))
        walk_nodes = walk_nodes[0] if isinstance(walk_nodes, tuple) else walk_nodes
        assert (walk_nodes > 0) == (name != "analytic" and form != "no_walk_tree"), (name, form, walk_nodes)
        n = 0
        for c in sr.CLASSES:
            rays, labels, flag, rec = cls[c]
            if rays.shape[0]:
                _compare(g, rays, flag, rec, f"{name} {form} {c}")
                n += rays.shape[0]
        assert n >= 4096
        parts = [cls[c] for c in sr.CLASSES if cls[c][0].shape[0]]
        rays = sr.interleaved([p[0] for p in parts])
        flag = sr.interleaved([p[2][:, None].astype(F32) for p in parts])[:, 0] != 0
        rec = sr.interleaved([p[3] for p in parts])
        assert rays.shape[0] == n
        _compare(g, rays, flag, rec, f"{name} {form} interleaved")
        if form == "default":                                      # (the helper the other query tests use, on one class: its own oracle pass)
            r = cls["slab_nan"][0][:512]
            query_and_compare(g, o, r, f"{name} slab_nan again")
    finally:
        g.close()


@pytest.fixture(scope="module")
def poses(seams):
    """seam_rays.frame_poses: each lies on the seam it names (test_seam_rays_cpu.py::test_frame_origins_lie_on_the_seams_they_name)"""
    return sr.frame_poses(lambda name: seams[name][1])


@pytest.mark.parametrize("k", range(sr.N_FRAME_POSES))
def test_frames_from_seam_origins(product_lib, oracle, poses, monkeypatch, k):
    """two frames at 48 x 16 from a camera position exactly on a seam, through the counting kernels and the timed ones, on both frame paths:
    every buffer of parity_util.compare_frame equal, and on the counting runs the six work counters"""
    name, what, pos, yaw, pitch = poses[k]
    pose = dict(pos=pos, yaw=yaw, pitch=pitch, fov=60.0)
    for path in ("w", "m"):
        for count in (True, False):
            _set_form(monkeypatch, None)
            monkeypatch.setenv("YCGE_PATH", path)
            o, g = pu.run_pair(oracle, sr.scene(name), 48, 16, 1, pose, frames=2, count=count)
            try:
                s = pu.compare_frame(o, g, check_counters=count)
                for key, v in s.items():
                    if key.endswith("_mismatch"):
                        assert v == 0, (name, what, path, count, key, v)
                if count:
                    for key in ("n_rays", "n_box", "n_tri", "n_prim", "n_vox", "n_rays_dark"):
                        assert s[key][0] == s[key][1], (name, what, path, key, s[key])
            finally:
                o.close(); g.close()
