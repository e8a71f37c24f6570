"""-m gpu: TAA without guide copies, and the cost feedback of trace_block without LDS round trips.

The synchronous single-device frame no longer copies this frame's normal, depth and sky flag into prev_* for the next frame's blend
(RaytraceRenderer.cs:380-396): it keeps the planes the trace wrote and traces the next frame into a second set (csrc/ycge_ctx.h:
guide_prev_*).  Every other frame form still copies, and a context may change form between any two frames.  Here three small scenes - one
per trace path - go through sequences of frames that change form, size, scene, frame counter and pose, and after EVERY frame the TAA
history, the guides (YCGE_BUF_PREV_*) and the frame's own planes (YCGE_BUF_G_NORMAL / G_DEPTH / SKY_MASK) are compared with the oracle bit
for bit.  YCGE_TAA_COPY_GUIDES=1 (the copying path, kept for A/B) must give the same bits.
(These sequences hold the guide HANDLING; the value edges of the blend itself - thresholds, non-finite and degenerate inputs - are held by the TAA probe, tests/test_gpu_taa_probe.py.)

Shapes: the smallest at which this can go wrong - frames that are no whole number of 32 x 8 tiles, more than one tile in both directions.
"""
import ctypes as C
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import parity_util as pu
from yetanotherconsolegameengine_amd import abi, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import flatten

pytestmark = pytest.mark.gpu

GUIDES = (("taa_history", abi.BUF_TAA_HISTORY), ("prev_normal", abi.BUF_PREV_NORMAL), ("prev_depth", abi.BUF_PREV_DEPTH), ("prev_sky", abi.BUF_PREV_SKY))
PLANES = (("g_normal", abi.BUF_G_NORMAL), ("g_depth", abi.BUF_G_DEPTH), ("sky", abi.BUF_SKY_MASK))
ORACLE_THREADS = 16

# name: (config, console width, console height, super-sampling, environment of the product's context)
CASES = {
    "console": (1, 40, 20, 1, {}),                            # 40 x 40 pixels: 2 x 5 tiles, the right-hand column 8 pixels wide; one launch, analytic walk
    "mesh": (3, 96, 27, 1, {"YCGE_LPT_ALWAYS": "1"}),         # 96 x 54: the bottom row of tiles 6 pixels high; k_trace, with the schedule behind every trace as on a full-size frame
    "voxel": (5, 72, 20, 2, {}),                              # 144 x 80: 5 x 10 tiles, the right-hand column 16 pixels wide; the stage pipeline
}


@lru_cache(maxsize=None)
def _scene(case):
    n, w, h, ss, env = CASES[case]
    sc, _, _, _, pose = scenes.config_scene(n, small=True, t01=0.5) if n == 5 else scenes.config_scene(n, small=True)
    return flatten(sc), sc, pose


class _Pair:
    """the oracle and the product's context side by side: every step goes to both, every frame is compared"""

    def __init__(self, oracle, case, monkeypatch, env=None, with_oracle=True):
        n, self.w, self.h, self.ss, case_env = CASES[case]
        for k in ("YCGE_PATH", "YCGE_TAA_COPY_GUIDES", "YCGE_TRACED_PACKET", "YCGE_LPT_ALWAYS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in {**case_env, **(env or {})}.items():
            monkeypatch.setenv(k, v)          # (the knobs are read once, in ycge_create)
        self.flat, sc, pose = _scene(case)
        self.pose = dict(pose)
        self.o = oracle.OracleRenderer(sc, self.w, self.h, self.ss, self.pose, flat=self.flat) if with_oracle else None
        self.g = RaytraceRenderer(self.flat, self.w, self.h, self.pose["fov"], self.ss)
        self.g.SetCamera(self.pose["pos"], self.pose["yaw"], self.pose["pitch"])
        self.case, self.frames, self.log = case, 0, []
        self._slab = self._hist = self._halo = None

    def close(self):
        if self.o is not None:
            self.o.close()
        self.g.close()

    # -- what a frame leaves, compared or recorded
    def check(self, label, planes=True):
        self.frames += 1
        which = GUIDES + (PLANES if planes else ())
        got = {name: self.g.read(buf) for name, buf in which}
        self.log.append((label, got))
        if self.o is None:
            return
        bad = {name: pu.mismatch_count(self.o.read(buf), got[name]) for name, buf in which}
        bad = {k: v for k, v in bad.items() if v}
        assert not bad, f"{self.case}: frame {self.frames} ({label}): {bad}"

    # -- steps
    def frame(self, label="synchronous"):
        if self.o is not None:
            self.o.render(stages=1, threads=ORACLE_THREADS)
        self.g.TryFlipAndBlit()
        self.check(label)
        return int(self.g.stats.history_reset)

    def frame_untimed(self):
        """the call a host makes that wants no statistics: no timing events, and the side stream's schedule waits for the stop event the
        trace launch itself carries (traced_ev)"""
        if self.o is not None:
            self.o.render(stages=1, threads=ORACLE_THREADS)
        rc = self.g.L.ycge_render_frame(self.g.ctx, None, None)
        assert rc == 0, rc
        self.check("synchronous, no statistics")

    def frame_sdr(self):
        """with the post stage, which reads the frame's planes behind TAA"""
        if self.o is not None:
            self.o.render(stages=2, threads=ORACLE_THREADS, want_sdr=True)
        self.g.TryFlipAndBlit(want_sdr=True)
        self.check("synchronous with an SDR buffer")

    def in_flight(self, n, check_each=False):
        for i in range(n):
            if self.o is not None:
                self.o.render(stages=1, threads=ORACLE_THREADS)
            self.g.RenderAsync()
            if check_each:
                self.check(f"in flight {i + 1}/{n}, joined")          # (a read-back joins the frames in flight)
        if not check_each:
            self.g.Wait()
            self.frames += n - 1
            self.check(f"the last of {n} in flight")

    def move(self, dx, dyaw=0.0):
        p = self.pose
        p["pos"] = (p["pos"][0] + dx, p["pos"][1], p["pos"][2]); p["yaw"] += dyaw
        if self.o is not None:
            self.o.set_camera(p["pos"], p["yaw"], p["pitch"], p["fov"])
        self.g.SetCamera(p["pos"], p["yaw"], p["pitch"])

    def resize(self, w, h, ss):
        if self.o is not None:
            self.o.resize(w, h, ss)
        self.g.Resize(w, h, ss)
        self._slab = self._hist = None

    def upload(self):
        self.g.UploadScene(self.flat)          # (RebuildBVH: the reference keeps its TAA state, and so does the oracle, which is not told)

    def counter(self, n):
        if self.o is not None:
            self.o.set_frame_counter(n)
        self.g.set_frame_counter(n)

    def tiled(self):
        """ycge_trace_tiles + ycge_resolve_gathered on this world of one: the slab form of the tiled frame"""
        import torch
        if self._slab is None:
            self._slab = torch.empty(self.g.tile_slab_bytes() // 4, dtype=torch.float32, device="cuda")
        if self.o is not None:
            self.o.render(stages=1, threads=ORACLE_THREADS)
        self.g.trace_tiles(self._slab.data_ptr(), 0)
        self.g.resolve_gathered(self._slab.data_ptr(), 0)
        self.check("tiled")

    def resident(self):
        """... and the tile-resident form (the frame's planes stay in its ring: only TAA's state is read back)"""
        import torch
        if self._hist is None:
            self._hist = torch.zeros(max(4, self.g.history_slab_bytes() // 4), dtype=torch.float32, device="cuda")
            self._halo = torch.zeros(16, dtype=torch.float32, device="cuda")
        if self.o is not None:
            self.o.render(stages=1, threads=ORACLE_THREADS)
        self.g.trace_tiles_resident(self._halo.data_ptr(), 0)
        self.g.resolve_tiles_resident(self._halo.data_ptr(), self._hist.data_ptr(), 0)
        self.check("tile-resident", planes=False)


def _static(p):
    for _ in range(6):          # both sets of planes three times
        p.frame()


def _pose_jump(p):
    p.frame(); p.frame()
    p.move(0.0005)          # below the reset threshold (TemporalAA.cs:58-67: 0.0025)
    assert p.frame("small move") == 0
    p.move(0.3, 0.2)
    assert p.frame("pose jump") == 1          # history reset: TAA does not read the guides
    assert p.frame("behind the jump") == 0
    p.frame()


def _sdr_between(p):
    p.frame(); p.frame_sdr(); p.frame(); p.frame_sdr(); p.frame_sdr(); p.frame()


def _in_flight_between(p):
    p.frame(); p.frame()
    p.in_flight(3)
    p.frame("synchronous behind frames in flight"); p.frame()
    p.in_flight(4)          # (an even number: the rotation of the three sets ends elsewhere)
    p.frame("synchronous behind frames in flight")
    p.in_flight(2, check_each=True)
    p.frame("synchronous behind frames in flight"); p.frame()


def _resize_between(p):
    w, h, ss = p.w, p.h, p.ss
    p.frame(); p.frame(); p.frame()
    p.resize(w - 7, h - 3, ss)
    p.frame("first of a new size"); p.frame(); p.frame()
    p.resize(w, h, ss)
    p.frame("first of the old size again"); p.frame()


def _upload_between(p):
    p.frame(); p.frame(); p.frame()
    p.upload()
    p.frame("behind a scene upload"); p.frame()
    p.upload(); p.upload()
    p.frame("behind two scene uploads")


def _counter_jumps(p):
    p.frame(); p.frame()
    p.counter(100)          # the next frame is 101: odd behind even twice
    p.frame("frame 101"); p.frame()
    p.counter(6)
    p.frame("frame 7"); p.frame(); p.frame()


def _untimed_between(p):
    p.frame(); p.frame_untimed(); p.frame("behind a frame without statistics")
    p.frame_untimed(); p.frame_untimed(); p.frame_untimed()
    p.frame("behind three frames without statistics"); p.frame()


def _tiled_between(p):
    p.frame(); p.frame()
    p.tiled(); p.tiled()
    p.frame("synchronous behind tiled frames"); p.frame()
    p.tiled()
    p.frame("synchronous behind a tiled frame")
    p.resident(); p.resident()
    p.frame("synchronous behind tile-resident frames"); p.frame()
    p.resident()
    p.tiled()
    p.frame()


SEQUENCES = {"static": _static, "pose_jump": _pose_jump, "sdr_between": _sdr_between, "in_flight_between": _in_flight_between, "resize_between": _resize_between,
             "upload_between": _upload_between, "counter_jumps": _counter_jumps, "tiled_between": _tiled_between, "untimed_between": _untimed_between}


@pytest.mark.parametrize("copy_guides", [False, True], ids=["default", "copy_guides"])
@pytest.mark.parametrize("sequence", list(SEQUENCES))
@pytest.mark.parametrize("case", list(CASES))
def test_guides_and_history_follow_the_oracle(product_lib, oracle, monkeypatch, case, sequence, copy_guides):
    """every frame of every sequence: TAA history, guides and the frame's planes bit-equal to the oracle's - by default and, the same sequences,
    under YCGE_TAA_COPY_GUIDES=1 (both equal to the oracle bit for bit, hence to each other)"""
    p = _Pair(oracle, case, monkeypatch, env={"YCGE_TAA_COPY_GUIDES": "1"} if copy_guides else None)
    try:
        SEQUENCES[sequence](p)
    finally:
        p.close()


def _everything(p):
    """one sequence with every change of form in it (the knob check: two contexts, no oracle)"""
    p.frame(); p.frame(); p.frame_sdr()
    p.move(0.0005); p.frame()
    p.in_flight(3)
    p.frame(); p.tiled(); p.frame(); p.resident(); p.frame()
    p.move(0.3, 0.2); p.frame(); p.frame()
    p.upload(); p.frame()
    p.counter(41); p.frame(); p.frame_sdr()
    p.resize(p.w - 7, p.h - 3, p.ss); p.frame(); p.frame(); p.in_flight(2); p.frame()


@pytest.mark.parametrize("case", list(CASES))
def test_copying_knob_changes_no_bit(product_lib, oracle, monkeypatch, case):
    """YCGE_TAA_COPY_GUIDES=1 - the synchronous frame copies the guides as before - and YCGE_TRACED_PACKET=1 - it records an event between the
    trace and TAA as before - against the default: the same buffers after every frame of a sequence that goes through every frame form."""
    logs = []
    for env in ({}, {"YCGE_TAA_COPY_GUIDES": "1"}, {"YCGE_TRACED_PACKET": "1"}):
        p = _Pair(oracle, case, monkeypatch, env=env, with_oracle=False)
        try:
            _everything(p)
        finally:
            p.close()
        logs.append(p.log)
    assert len(logs[0]) == len(logs[1]) == len(logs[2]) > 15
    for other, name in ((logs[1], "YCGE_TAA_COPY_GUIDES=1"), (logs[2], "YCGE_TRACED_PACKET=1")):
        for i, ((label, a), (_, b)) in enumerate(zip(logs[0], other)):
            bad = [k for k in a if not pu.bits_equal(a[k], b[k])]
            assert not bad, f"{case}: {name}: frame {i + 1} ({label}): {bad}"


# ------------------------------------------------------------------------------------------------ trace_block: the light loop, the cost feedback
def _many_lights_scene():
    """A floor, a wall and a coarse sphere mesh under five point lights.  One light lies BELOW the floor and one BEHIND the wall: for the hits
    on those surfaces n . l <= 0, the light-loop head skips them (RaytraceRenderer.cs:584) and the contribution code of the NEXT light follows
    the answer of its shadow ray; the mesh's underside faces see the light below the floor.  Shadow rays of the floor cross the mesh."""
    from yetanotherconsolegameengine_amd.scene import AmbientLight, Checker, Material, Mesh, Plane, PointLight, Scene, vec3
    th = np.linspace(0.1, np.pi - 0.1, 9); ph = np.linspace(0, 2 * np.pi, 12, endpoint=False)
    P = np.array([[np.sin(t) * np.cos(p), np.cos(t), np.sin(t) * np.sin(p)] for t in th for p in ph], np.float32) * np.float32(0.7) + np.array([0.1, 1.0, -3.0], np.float32)
    tris = []
    for i in range(len(th) - 1):
        for j in range(len(ph)):
            a, b = i * len(ph) + j, i * len(ph) + (j + 1) % len(ph)
            tris += [[P[a], P[b], P[a + len(ph)]], [P[b], P[b + len(ph)], P[a + len(ph)]]]
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.04)
    s.Objects.append(Plane(vec3(0, 0, 0), vec3(0, 1, 0), Checker(vec3(0.8, 0.8, 0.8), vec3(0.3, 0.3, 0.3), 0.5), 0.0, 0.0))
    s.Objects.append(Plane(vec3(0, 0, -6.0), vec3(0, 0, 1), Material(vec3(0.7, 0.6, 0.5)), 0.0, 0.0))
    s.Objects.append(Mesh(np.array(tris, np.float32), Material(vec3(0.8, 0.45, 0.25))))
    s.Lights.append(PointLight(vec3(0.5, -2.0, -3.0), vec3(1.0, 0.9, 0.8), 60.0))          # below the floor: first in the list, skipped for every floor hit
    s.Lights.append(PointLight(vec3(1.5, 5.0, -1.0), vec3(1, 1, 1), 70.0))
    s.Lights.append(PointLight(vec3(0.0, 2.0, -9.0), vec3(0.8, 0.9, 1.0), 90.0))           # behind the wall: in the middle of the list
    s.Lights.append(PointLight(vec3(-3.0, 3.0, -2.0), vec3(0.9, 0.95, 1.0), 40.0))
    s.Lights.append(PointLight(vec3(-0.5, 0.15, -1.5), vec3(1.0, 0.6, 0.6), 5.0))          # grazing the floor, under the mesh
    return s, dict(pos=(0.2, 1.3, 0.6), yaw=0.03, pitch=-0.12, fov=55.0)


@pytest.mark.parametrize("count", [False, True])
def test_light_loop_head_and_contribution_with_skipped_lights(product_lib, oracle, monkeypatch, count):
    """trace_block's light-loop head (:578-591) queues a shadow ray for a light and the contribution code (:592-602) adds that light one trip
    later, with lights skipped in between (n . l <= 0): current_hdr bit-equal to the oracle's on a 64 x 32 console with five lights, two of them
    behind a surface; k_trace<false, true> (what is timed) and the counting instance.  (Parking the head's values for the contribution code
    was measured and not kept - DESIGN.md section 8; the test holds whatever form that pair of code takes.)"""
    monkeypatch.delenv("YCGE_PATH", raising=False)
    sc, pose = _many_lights_scene()
    o, g = pu.run_pair(oracle, sc, 64, 32, 1, pose, frames=1, oracle_threads=ORACLE_THREADS, count=count)
    try:
        for f in range(3):          # (the bounce rays differ from frame to frame)
            if f:
                o.render(stages=1, threads=ORACLE_THREADS); g.TryFlipAndBlit()
            st = pu.compare_frame(o, g, check_counters=count)
            print("frame", f + 1, {k: v for k, v in st.items() if k.endswith("_mismatch") and v})
            assert st["current_hdr_mismatch"] == 0 and st["taa_history_mismatch"] == 0 and st["rng_state_mismatch"] == 0
            if count:
                assert st["n_rays"][0] == st["n_rays"][1] and st["n_rays_dark"][0] == st["n_rays_dark"][1]
        hdr = g.read(abi.BUF_CURRENT_HDR)
        assert (hdr.reshape(-1, 3).max(axis=1) > 0).mean() > 0.5
    finally:
        o.close(); g.close()


def test_block_costs_are_what_they_were(product_lib, monkeypatch):
    """A block's cost for the schedule - the sum over its trips of the longest lane's traversal steps - is now found with the vector ALU's lane
    crossbar instead of six exchanges through the LDS (wave_umax).  One frame of the mesh case, costs read through the per-wavefront profile
    record (ycge_debug_read_wave_prof): equal, block for block, to what the build before the change recorded (tests/golden/block_costs_mesh_96x27.npy)."""
    monkeypatch.setenv("YCGE_WAVE_PROF", "mega"); monkeypatch.setenv("YCGE_PATH", "megakernel")
    flat, sc, pose = _scene("mesh")
    _, w, h, ss, _ = CASES["mesh"]
    g = RaytraceRenderer(flat, w, h, pose["fov"], ss)
    try:
        g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        g.TryFlipAndBlit()
        n_tiles = ((g.hiW + 31) // 32) * ((g.hiH + 7) // 8)
        buf = np.zeros(n_tiles * 16, dtype=np.uint64)
        g.L.ycge_debug_read_wave_prof.restype = C.c_int
        g.L.ycge_debug_read_wave_prof.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        assert g.L.ycge_debug_read_wave_prof(g.ctx, buf.ctypes.data, buf.size) == 0
    finally:
        g.close()
    cost = (buf.reshape(-1, 4)[:, 2] >> np.uint64(32)).astype(np.uint32)
    want = np.load(Path(__file__).resolve().parent / "golden" / "block_costs_mesh_96x27.npy")
    assert cost.shape == want.shape and want.max() > 64 and (want > 0).sum() > 16          # (the fixture is a frame with work in it)
    assert np.array_equal(cost, want), f"{int((cost != want).sum())} of {cost.size} block costs differ"
