"""The post-stage kernels (csrc/ycge_post.hip) through their hooks on inputs no rendered frame produces.

ycge_test_exposure runs the exposure sum kernels alone on drawn log terms: logSum bit for bit against a plain binary32 serial loop, cnt, and
both exposure values against the oracle's UpdateExposure tail (orc_exposure_probe) - for the chunked form (k_exposure_chunk_sums, _prefix,
_chunk_maps, k_exposure_sum) and for YCGE_EXPOSURE_SERIAL (k_exposure_sum_serial), around one chunk of 512, one group of 16 chunks, one batch of
1024 chunks and three batches.

ycge_test_post_stage runs the frames' own run_post on drawn trace grids (tests/post_probe_inputs.py): denoised image, logSum, cnt, both exposure
values and the SDR array against the oracle's post stage (orc_post_probe_sums, itself held to a Python restatement on the same families by
tests/test_oracle_kats.py).  Everything is compared bit for bit, a NaN counting as equal to any NaN.

Which case reaches which kernel form (run_post, csrc/ycge_post_host.cpp): iteration 0 and every even iteration are the plain k_atrous; with
config.atrous_inplace_exact = 1 the odd iterations (steps 2 and 8) run in place behind k_atrous_static:
  "split"      default knobs, a grid of 24 rows or more: step 2 is the persistent k_atrous_stream<16, DUO> over row-parity half-bands;
  "whole"      YCGE_POST_NO_SPLIT=1 (and every grid below 24 rows, and step 8): the persistent k_atrous_stream<16> over whole bands, LDS window;
  "block"      YCGE_POST_MODE=3: the persistent forms with bands in block order (tickets);
  "launch"     YCGE_POST_MODE=2: k_atrous_band<16, window> with a launch per level group;
  "hash"       YCGE_POST_MODE=2 YCGE_POST_HASH_FORM=1: k_atrous_band<16, hash>;
  "waived"     atrous_inplace_exact = 0: k_atrous only; this case also sets YCGE_EXPOSURE_SERIAL (k_exposure_sum_serial inside a frame's post).
Five iterations add the in-place step 8 (bands of 16 rows); one iteration makes exposure and tone map read the history itself.
k_exposure_terms, the chunked sum and k_tonemap_downsample (ss 1, 2, 3) run in every case."""
import os

import numpy as np
import pytest

import post_probe_inputs as ppi
from yetanotherconsolegameengine_amd import abi, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import flatten

pytestmark = pytest.mark.gpu
F32 = np.float32
KNOBS = ("YCGE_POST_MODE", "YCGE_POST_NO_SPLIT", "YCGE_POST_HASH_FORM", "YCGE_EXPOSURE_SERIAL")
FORMS = {
    "split": {}, "whole": {"YCGE_POST_NO_SPLIT": "1"}, "block": {"YCGE_POST_MODE": "3"}, "block_whole": {"YCGE_POST_MODE": "3", "YCGE_POST_NO_SPLIT": "1"},
    "launch": {"YCGE_POST_MODE": "2"}, "launch_whole": {"YCGE_POST_MODE": "2", "YCGE_POST_NO_SPLIT": "1"},
    "hash": {"YCGE_POST_MODE": "2", "YCGE_POST_HASH_FORM": "1"}, "waived": {"YCGE_EXPOSURE_SERIAL": "1"},
}


def make_renderer(monkeypatch, fbw, fbh, ss, iters=3, phi=ppi.DEFAULT_PHI, exact=1, env=None, scene=None, **kw):
    """a context whose knobs were read with `env` set (ycge_create reads every YCGE_* knob once)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    cfg = abi.default_config()
    cfg.atrous_iterations, cfg.atrous_inplace_exact = iters, exact
    cfg.atrous_c_phi, cfg.atrous_n_phi, cfg.atrous_z_phi, cfg.atrous_a_phi = [float(p) for p in phi]
    g = RaytraceRenderer(scene, fbw, fbh, 45.0, ss, cfg=cfg, **kw)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return g


def compare_post(got, want, what):
    """(denoised, sdr, state) of the device against the oracle's: the number of differences per quantity, printed, all zero"""
    (den_g, sdr_g, st_g), (den_o, sdr_o, st_o) = got, want
    bad = dict(denoised=ppi.nan_aware_mismatches(den_g, den_o), sdr=ppi.nan_aware_mismatches(sdr_g, sdr_o),
               log_sum=int(not ppi.same_f32(st_g["log_sum"], st_o["log_sum"])), count=int(st_g["count"] != st_o["count"]),
               ae_exposure=int(not ppi.same_f32(st_g["ae_exposure"], st_o["ae_exposure"])), effective=int(not ppi.same_f32(st_g["effective"], st_o["effective"])))
    print(what, "differences", bad, "device", {k: st_g[k] for k in ("log_sum", "count", "ae_exposure", "serial_chunks")}, "oracle", st_o)
    assert not any(bad.values()), (what, bad, st_g, st_o)


# ------------------------------------------------------------------------------------------------------------- 1: the exposure kernels alone
@pytest.fixture(scope="module")
def expo_ctx(product_lib):
    g = RaytraceRenderer(None, 16, 8, 45.0, 1)
    yield g
    g.close()


def check_exposure(g, oracle, family, n, ae0, seed=0):
    terms = ppi.exposure_terms(family, n, seed)
    ref_sum, ref_cnt = ppi.serial_sum_f32(terms), int(np.count_nonzero(terms))
    st_o = oracle.exposure_probe(terms, ae0)
    assert ppi.same_f32(st_o["log_sum"], ref_sum) and st_o["count"] == ref_cnt, (family, n, st_o, ref_sum, ref_cnt)      # (the two references agree)
    n_chunks = (n + 511) // 512
    for serial in (False, True):
        st = g.exposure_probe(terms, ae0, serial=serial)
        what = (family, n, ae0, "serial" if serial else "chunked")
        print(*what, "log_sum", st["log_sum"], "count", st["count"], "ae", st["ae_exposure"], "chunks added one by one", st["serial_chunks"], "of", n_chunks)
        assert ppi.same_f32(st["log_sum"], ref_sum), (what, st, ref_sum)
        assert st["count"] == ref_cnt, (what, st, ref_cnt)
        assert ppi.same_f32(st["ae_exposure"], st_o["ae_exposure"]) and ppi.same_f32(st["effective"], st_o["effective"]), (what, st, st_o)
        if serial:
            assert st["serial_chunks"] == 0
        elif family in ppi.EXPOSURE_TAME and n >= 131072:
            # The fast path must carry the bulk: a sum of these terms passes at most ~36 binades on its way from 2^-12 to its end (< 2^24), and a
            # crossing costs the chunk it happens in and at most the next; the first chunk is always added one by one.  Far below a third of
            # the 1024 chunks and more these lengths have - a kernel that silently always falls back is noticed (the twin's bound,
            # tests/test_exposure_chunked_sum.py).
            assert st["serial_chunks"] < n_chunks // 3, (what, st["serial_chunks"], n_chunks)


@pytest.mark.parametrize("family", ppi.EXPOSURE_FAMILIES)
def test_exposure_kernels_alone(expo_ctx, oracle, family):
    """every term family at every length (one chunk, one group, one batch, each +-1; three batches with a ragged last chunk), both forms;
    the starting exposure walks through 0.1, 1.0, 1.5 and NaN"""
    for k, n in enumerate(ppi.EXPOSURE_LENGTHS):
        check_exposure(expo_ctx, oracle, family, n, [1.0, 0.1, 1.5, float("nan")][(k + ppi.EXPOSURE_FAMILIES.index(family)) % 4])


def test_exposure_every_starting_value_on_clamped_and_unclamped_sums(expo_ctx, oracle):
    """bright (target clamps to aeMin), dark (aeMax), no samples (target = aeExposure) and an unclamped mean, each from 0.1, 1.0, 1.5 and NaN"""
    for ae0 in (0.1, 1.0, 1.5, float("nan")):
        for family in ("bright", "dark", "all_zero", "hover_zero", "nan_mid"):
            check_exposure(expo_ctx, oracle, family, 8193, ae0, seed=3)
        terms = np.log(F32(1e-6) + np.random.default_rng(9).uniform(0.1, 0.9, 4000).astype(F32)).astype(F32)          # mean log luminance in [-2, 0.5]
        st_o = oracle.exposure_probe(terms, ae0)
        for serial in (False, True):
            st = expo_ctx.exposure_probe(terms, ae0, serial=serial)
            assert ppi.same_f32(st["log_sum"], st_o["log_sum"]) and st["count"] == st_o["count"] and ppi.same_f32(st["effective"], st_o["effective"]), (ae0, serial, st, st_o)
        if ae0 == 1.0: assert 0.10 < float(st_o["ae_exposure"]) < 1.5 and float(st_o["ae_exposure"]) != 1.0


def test_exposure_hook_refusals(expo_ctx):
    for terms in (np.zeros(0, F32),):
        with pytest.raises(abi.YcgeError) as e:
            expo_ctx.exposure_probe(terms)
        assert e.value.status == abi.YCGE_ERR_INVALID_ARG
    assert expo_ctx.exposure_probe(np.ones(5, F32))["count"] == 5          # ... and the context is none the worse for it


# ------------------------------------------------------------------------------------------------------------- 2: the whole post stage
# (fbw, fbh, ss, iterations, exact, form): trace grid fbw ss x 2 fbh ss
POST_CASES = [
    (192, 54, 1, 3, 1, "split"), (192, 54, 1, 3, 1, "whole"), (192, 54, 1, 3, 1, "launch"), (192, 54, 1, 3, 1, "hash"), (192, 54, 1, 3, 1, "block"),
    (131, 37, 1, 5, 1, "split"), (131, 37, 1, 5, 1, "launch_whole"), (131, 37, 1, 5, 1, "hash"),
    (64, 20, 2, 2, 1, "split"), (64, 20, 2, 3, 0, "waived"), (64, 20, 2, 5, 1, "block_whole"),
    (33, 10, 1, 1, 1, "split"), (33, 10, 1, 3, 1, "block"), (33, 10, 1, 2, 1, "launch"),
    (1, 1, 1, 3, 1, "split"), (1, 1, 1, 5, 1, "launch"), (1, 1, 1, 2, 0, "waived"),
    (11, 7, 3, 3, 1, "split"), (11, 7, 3, 2, 0, "waived"), (11, 7, 3, 5, 1, "hash"),
    (24, 150, 1, 3, 1, "split"), (24, 150, 1, 3, 1, "block"),          # 300 rows: the persistent form hands over across 70-odd half-bands
]
_oracle_cache = {}


def oracle_post(oracle, fbw, fbh, ss, d, iters, exact, ae0, key):
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle.post_probe(fbw, fbh, ss, d["hdr"], d["alb"], d["nrm"], d["dep"], d["sky"], iters, d["phi"], ae0, exact)
    return _oracle_cache[key]


@pytest.mark.parametrize("case", POST_CASES, ids=lambda c: "%dx%d_ss%d_it%d_%s%s" % (c[0], c[1], c[2], c[3], c[5], "" if c[4] else "_pingpong"))
def test_post_stage_every_family(product_lib, oracle, monkeypatch, case):
    """every input family of tests/post_probe_inputs.py through one kernel form each (see the module's text), on one context per phi setting:
    the families follow each other on the SAME context, so schedule cache, persistent-launch epochs and tickets carry over as between frames."""
    fbw, fbh, ss, iters, exact, form = case
    W, H = fbw * ss, fbh * 2 * ss
    ctxs = {}
    try:
        for k, family in enumerate(ppi.FAMILIES):
            d = ppi.make_inputs(family, W, H, seed=7)
            ae0 = [1.0, 0.1, 1.5, float("nan")][k % 4]
            if d["phi"] not in ctxs:
                ctxs[d["phi"]] = make_renderer(monkeypatch, fbw, fbh, ss, iters, d["phi"], exact, FORMS[form])
            got = ctxs[d["phi"]].post_probe(d["hdr"], d["alb"], d["nrm"], d["dep"], d["sky"], ae0)
            want = oracle_post(oracle, fbw, fbh, ss, d, iters, exact, ae0, (family, fbw, fbh, ss, iters, exact, ae0))
            compare_post(got, want, f"{family} {W}x{H} ss{ss} {iters} iterations {form}")
            if family in ppi.TAME_FAMILIES and W * H // (max(2, 2 * ss) ** 2) >= 131072:
                assert got[2]["serial_chunks"] < (W * H // (max(2, 2 * ss) ** 2) + 511) // 512 // 3
    finally:
        for g in ctxs.values():
            g.close()


def test_post_stage_carries_the_exposure_and_recovers_from_poison(product_lib, oracle, monkeypatch):
    """Three calls in a row on one context, each starting from the exposure the call before left (as frames do); then a poisoned call (NaN
    radiance: NaN exposure) followed by two clean ones - against the oracle's chain."""
    fbw, fbh, ss = 64, 20, 1
    g = make_renderer(monkeypatch, fbw, fbh, ss)
    try:
        for chain in (("tame", "sky_checker", "constant_one_changed"), ("nonfinite_rows", "tame", "depth_equal")):
            ae_g = ae_o = 1.0
            for family in chain:
                d = ppi.make_inputs(family, fbw * ss, fbh * 2 * ss, seed=11)
                got = g.post_probe(d["hdr"], d["alb"], d["nrm"], d["dep"], d["sky"], ae_g)
                want = oracle.post_probe(fbw, fbh, ss, d["hdr"], d["alb"], d["nrm"], d["dep"], d["sky"], 3, d["phi"], ae_o, 1)
                compare_post(got, want, f"chain {chain} at {family}")
                ae_g, ae_o = got[2]["ae_exposure"], want[2]["ae_exposure"]
    finally:
        g.close()


def test_probe_between_two_frames_leaves_the_second_frame_a_twin_contexts(product_lib, oracle, monkeypatch):
    """ycge_test_post_stage dirties the TAA history, the G-buffer (albedo, normal, depth, sky), the denoise buffers and the exposure state - and
    nothing else.  A context that is probed between two frames, gets its exposure put back (a probe of an all-sky image counts no sample:
    the state stays at its ae_in) and its history reset (Resize to the same size) renders the second frame as a twin context that was only
    resized: every buffer, the exposure and the SDR array."""
    sc, _, _, _, pose = scenes.config_scene(1)
    flat = flatten(sc)
    fbw, fbh, ss = 48, 14, 1
    pair = [make_renderer(monkeypatch, fbw, fbh, ss, scene=flat, capture_debug=True) for _ in range(2)]
    try:
        for r in pair:
            r.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        s1 = [r.TryFlipAndBlit(want_sdr=True) for r in pair]
        assert ppi.nan_aware_mismatches(s1[0], s1[1]) == 0
        e1 = F32(pair[0].stats.exposure)
        d = ppi.make_inputs("nonfinite_isolated", fbw * ss, fbh * 2 * ss, seed=5)
        den, sdr, st = pair[0].post_probe(d["hdr"], d["alb"], d["nrm"], d["dep"], d["sky"], 0.7)
        assert np.isnan(sdr).any() or np.isnan(den).any()
        _, _, st = pair[0].post_probe(d["hdr"], d["alb"], d["nrm"], d["dep"], np.ones_like(d["sky"]), e1)          # puts the exposure back
        assert st["count"] == 0 and ppi.same_f32(st["ae_exposure"], e1) and ppi.same_f32(st["effective"], e1)
        for r in pair:
            r.Resize(fbw, fbh, ss)
        s2 = [r.TryFlipAndBlit(want_sdr=True) for r in pair]
        for which in (abi.BUF_RAYS, abi.BUF_CURRENT_HDR, abi.BUF_G_ALBEDO, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK, abi.BUF_TAA_HISTORY, abi.BUF_DENOISED):
            a, b = pair[0].read(which), pair[1].read(which)
            assert (ppi.nan_aware_mismatches(a, b) if a.dtype.kind == "f" else int(np.count_nonzero(a != b))) == 0, which
        assert ppi.same_f32(pair[0].stats.exposure, pair[1].stats.exposure) and float(pair[0].stats.exposure) != float(e1)
        assert ppi.nan_aware_mismatches(s2[0], s2[1]) == 0 and np.isfinite(s2[0]).all()
    finally:
        for r in pair:
            r.close()


def test_post_hook_refusals_leave_the_context_usable(product_lib, oracle, monkeypatch):
    """frames in flight and a rank of several are refused (YCGE_ERR_INVALID_ARG, a message that says why); so is an array of the wrong size by
    the wrapper; afterwards the same context renders and probes as before"""
    sc, _, _, _, pose = scenes.config_scene(1)
    fbw, fbh, ss = 32, 9, 1
    d = ppi.make_inputs("tame", fbw, fbh * 2, seed=2)
    g = make_renderer(monkeypatch, fbw, fbh, ss, scene=flatten(sc))
    try:
        g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        g.RenderAsync()
        with pytest.raises(abi.YcgeError, match="in flight") as e:
            g.post_probe(d["hdr"], d["alb"], d["nrm"], d["dep"], d["sky"])
        assert e.value.status == abi.YCGE_ERR_INVALID_ARG
        with pytest.raises(abi.YcgeError, match="in flight"):
            g.exposure_probe(np.ones(4, F32))
        g.Wait()
        with pytest.raises(ValueError):
            g.post_probe(d["hdr"][:-1], d["alb"], d["nrm"], d["dep"], d["sky"])
        got = g.post_probe(d["hdr"], d["alb"], d["nrm"], d["dep"], d["sky"])
        compare_post(got, oracle.post_probe(fbw, fbh, ss, d["hdr"], d["alb"], d["nrm"], d["dep"], d["sky"]), "after the refusals")
        assert np.isfinite(g.TryFlipAndBlit(want_sdr=True)).all()
    finally:
        g.close()
    r = make_renderer(monkeypatch, fbw, fbh, ss, rank=1, world_size=2)
    try:
        with pytest.raises(abi.YcgeError, match="rank 1 of 2") as e:
            r.post_probe(d["hdr"], d["alb"], d["nrm"], d["dep"], d["sky"])
        assert e.value.status == abi.YCGE_ERR_INVALID_ARG
    finally:
        r.close()
