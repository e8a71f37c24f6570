"""TemporalBlendWithClamp's two references against each other, and the conditions the drawn inputs must meet - no GPU.

The oracle's Renderer::temporal_blend (orc_taa_probe) runs against the independent binary32 restatement (py_restatement.temporal_blend) on every
input family of tests/taa_probe_inputs.py, bit for bit, a NaN equal to any NaN: what tests/test_gpu_taa_probe.py holds the kernels to is
itself held here.

The conditions are asserted on the restatement's own report of the branches it took (which alpha branch, which clamp branch, how many taps of
the window matched), so the GPU test cannot pass on inputs that skip a branch: over `tame` every branch is taken by at least 32 pixels,
every special family puts at least 32 pixels on the branches it is named for, `sky_edges` produces every count of matching taps from 1 to 9,
the threshold pairs land on 0.05 / 0.8 and both their binary32 neighbours, no output is NaN outside the families that feed NaN or make it,
and inside them at most half of the history is."""
import numpy as np
import pytest

import py_restatement as pr
import taa_probe_inputs as tpi

f32 = np.float32
OUT_KEYS = ("hist", "prev_normal", "prev_depth", "prev_sky")
SMALL = (13, 11)
BIG = (40, 40)


def restated(d, reset, alpha, radius, pad, branches=None):
    state = dict(hist=d["hist"].copy(), prev_normal=d["pnrm"].copy(), prev_depth=d["pdep"].copy(), prev_sky=d["psky"].copy())
    with np.errstate(all="ignore"):
        pr.temporal_blend(state, d["cur"], d["nrm"], d["dep"], d["sky"], bool(reset), alpha, radius, pad, branches=branches)
    return state


def compare(got, want, what):
    bad = {k: tpi.nan_aware_mismatches(got[k], want[k]) for k in OUT_KEYS}
    assert not any(bad.values()), (what, bad)


def check_nan_rule(family, out, what):
    nans = int(np.isnan(out["hist"]).sum())
    if family in tpi.NAN_FAMILIES:
        assert nans * 2 <= out["hist"].size, (what, nans, out["hist"].size)
    else:
        assert nans == 0 and not np.isnan(out["prev_normal"]).any() and not np.isnan(out["prev_depth"]).any(), (what, nans)


def test_the_walk_reaches_every_parameter_value():
    sets = [tpi.walk(k) for k in range(48)]
    assert {s[0] for s in sets} == set(tpi.ALPHAS) and {s[1:] for s in sets} == {(r, p) for r in tpi.RADII for p in tpi.PADS}
    tile = [tpi.walk(k, tile_form=True) for k in range(48)]
    assert {s[1] for s in tile} == {0, 1} and {s[2] for s in tile} == set(tpi.PADS) and {s[0] for s in tile} == set(tpi.ALPHAS)
    # what the device test draws from it (tests/test_gpu_taa_probe.py).  Plane forms: the six sets a family walks over its shapes hold every
    # alpha and every radius, and at ANY ONE shape the families between them meet every alpha and every radius too
    for family in tpi.FAMILIES:
        six = [tpi.family_walk(family, k) for k in range(6)]
        assert {s[0] for s in six} == set(tpi.ALPHAS) and {s[1] for s in six} == set(tpi.RADII)
    for k in range(6):
        at_shape = [tpi.family_walk(f, k) for f in tpi.FAMILIES]
        assert {s[0] for s in at_shape} == set(tpi.ALPHAS) and {s[1] for s in at_shape} == set(tpi.RADII), (k, at_shape)
    # Tile forms: on EVERY rank every family has a blend (no reset) at radius 1 - the one radius at which halo records are read - and a call at
    # radius 0; over the families a rank meets every alpha and every pad at radius 1, and both a reset and a blend at radius 0
    for rank in range(8):
        per_family = {f: tpi.tile_cases(f, rank) for f in tpi.FAMILIES}
        for f, cases in per_family.items():
            assert [c for c in cases if c[0] == 0 and c[2] == 1] and [c for c in cases if c[2] == 0], (rank, f, cases)
            assert all(c[2] in (0, 1) for c in cases)
        halo = [c for cases in per_family.values() for c in cases if c[0] == 0 and c[2] == 1]
        assert {c[1] for c in halo} == set(tpi.ALPHAS) and {c[3] for c in halo} == set(tpi.PADS), (rank, halo)
        assert {c[0] for cases in per_family.values() for c in cases if c[2] == 0} == {0, 1}, rank


@pytest.mark.parametrize("family", tpi.FAMILIES)
def test_oracle_against_the_restatement_over_the_walk(oracle, family):
    W, H = SMALL
    d = tpi.make_inputs(family, W, H, seed=3)
    for k in range(6):
        alpha, radius, pad = tpi.family_walk(family, k)
        for reset in ((0, 1) if k == 0 else (0,)):
            want = restated(d, reset, alpha, radius, pad)
            got = oracle.taa_probe(reset, *tpi.planes(d), alpha, radius, pad)
            compare(got, want, (family, alpha, radius, pad, reset))
            check_nan_rule(family, want, (family, alpha, radius, pad, reset))
            if reset:
                assert tpi.nan_aware_mismatches(got["hist"], d["cur"]) == 0 and tpi.nan_aware_mismatches(got["prev_depth"], d["dep"]) == 0
    # every call leaves this frame's normal, depth and sky flag as the next frame's guides
    assert tpi.nan_aware_mismatches(got["prev_normal"], d["nrm"]) == 0 and tpi.nan_aware_mismatches(got["prev_sky"], d["sky"]) == 0


@pytest.mark.parametrize("family", tpi.FAMILIES)
def test_conditions_on_the_restatements_branches(oracle, family):
    W, H = BIG
    d = tpi.make_inputs(family, W, H, seed=7)
    br = {}
    want = restated(d, 0, 0.01, 1, 0.10, br)
    compare(oracle.taa_probe(0, *tpi.planes(d), 0.01, 1, 0.10), want, family)
    check_nan_rule(family, want, family)
    counts = {(which, code): int(np.count_nonzero(br[which] == code)) for which, code in tpi.FAMILY_BRANCHES[family]}
    print(family, "pixels per branch", counts, "NaN history values", int(np.isnan(want["hist"]).sum()))
    assert all(v >= 32 for v in counts.values()), (family, counts)
    assert br["taps"].min() >= 1 and br["taps"].max() <= 9
    if family == "sky_edges":
        taps = {int(t): int(np.count_nonzero(br["taps"] == t)) for t in range(1, 10)}
        print("matching taps", taps)
        assert all(v > 0 for v in taps.values()), taps
    if family == "thresholds":
        lo, at, hi = tpi._neighbours(0.05)
        rel = tpi.rel_f32(d["dep"], d["pdep"])
        n_lo, n_at, n_hi = (int(np.count_nonzero(rel == t)) for t in (lo, at, hi))
        assert min(n_lo, n_at, n_hi) >= 16, (n_lo, n_at, n_hi)
        assert np.all(br["alpha"][rel == hi] == pr.TAA_ALPHA_REL) and np.all(br["alpha"][(rel == at) | (rel == lo)] == pr.TAA_ALPHA_KEPT)
        lo, at, hi = tpi._neighbours(0.8)
        nd = tpi.ndot_f32(d["nrm"], d["pnrm"])
        n_lo, n_at, n_hi = (int(np.count_nonzero(nd == t)) for t in (lo, at, hi))
        assert min(n_lo, n_at, n_hi) >= 16, (n_lo, n_at, n_hi)
        assert np.all(br["alpha"][nd == lo] == pr.TAA_ALPHA_NDOT) and np.all(br["alpha"][(nd == at) | (nd == hi)] == pr.TAA_ALPHA_KEPT)
        floor = np.minimum(d["dep"], d["pdep"]) <= f32(1e-4)          # at and under the floor, zero and negative: both verdicts occur
        assert np.count_nonzero(floor & (br["alpha"] == pr.TAA_ALPHA_REL)) >= 16 and np.count_nonzero(floor & (br["alpha"] == pr.TAA_ALPHA_KEPT)) >= 16
    if family == "luminance":
        pl = tpi.luma_f32(d["hist"])
        assert np.count_nonzero(pl == 0) >= 16 and np.count_nonzero((pl > 0) & (pl < f32(1e-6))) >= 16 and np.count_nonzero(pl < 0) >= 16
        assert np.count_nonzero(np.isinf(pl)) >= 8
    if family == "nan_colours":
        assert np.isnan(d["cur"]).any() and np.isinf(d["cur"]).any() and np.isnan(want["hist"]).sum() >= 32


def test_branch_report_leaves_the_result_alone():
    d = tpi.make_inputs("tame", *SMALL, seed=1)
    a, b = restated(d, 0, 0.5, 2, 0.1), restated(d, 0, 0.5, 2, 0.1, {})
    compare(a, b, "with and without the report")
