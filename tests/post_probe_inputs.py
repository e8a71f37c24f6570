"""Inputs for the post stage (steps 6-8 of TryFlipAndBlit) that no rendered frame produces, drawn by seed: shared by the CPU test that
holds the oracle's post stage to its Python restatement (test_oracle_kats.py) and the GPU tests that hold the kernels to the oracle
(test_gpu_post_probe.py).  Every family returns dict(hdr, alb, nrm, dep, sky, phi) for a W x H trace grid; `phi` is what the config's four
atrous_*_phi are set to."""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(f32).max
DEFAULT_PHI = (3.0, 0.35, 2.0, 0.20)
# finite values a sane frame never holds / values that are not finite
FINITE_SPECIALS = [FLT_MAX, -FLT_MAX, f32(1e30), f32(-1e30), f32(1e-40), f32(-1e-40), f32(-0.0), f32(-1.5), f32(1e-38), f32(65504.0)]
NONFINITE_SPECIALS = [f32(np.nan), f32(np.inf), f32(-np.inf)]

FAMILIES = (
    "tame", "sky_none", "sky_all", "sky_checker", "sky_single_nonsky", "sky_band_rows",
    "constant", "constant_one_changed", "phi_zero", "phi_negative", "phi_tiny",
    "normals_zero", "normals_nonunit", "normals_overflow", "depth_inf", "depth_equal", "all_dark",
    "finite_isolated", "finite_rows", "finite_corner", "finite_band_edge", "finite_self_tap",
    "nonfinite_isolated", "nonfinite_rows", "nonfinite_corner", "nonfinite_band_edge", "nonfinite_self_tap",
)
# families whose exposure terms are ordinary (the fast path of the chunked sum must carry them)
TAME_FAMILIES = ("tame", "sky_none", "sky_checker", "constant", "normals_nonunit", "depth_equal")


def _base(W, H, rng):
    hdr = rng.uniform(0, 2.5, (H, W, 3)).astype(f32)
    alb = rng.uniform(0, 1, (H, W, 3)).astype(f32)
    nrm = rng.normal(size=(H, W, 3)).astype(f32)
    dep = rng.uniform(1, 9, (H, W)).astype(f32)
    sky = (rng.uniform(size=(H, W)) < 0.2).astype(np.uint8)
    hdr[sky == 1] = f32(0.7)
    return dict(hdr=hdr, alb=alb, nrm=nrm, dep=dep, sky=sky, phi=DEFAULT_PHI)


def _places(kind, W, H, rng):
    """pixel lists [(y, x)] for the placements of the special values"""
    if kind == "isolated":
        k = max(1, min(W * H, (W * H) // 37 + 3))
        idx = rng.choice(W * H, size=k, replace=False)
        return [(int(i // W), int(i % W)) for i in idx]
    if kind == "rows":          # whole rows: the first, one inside, the last
        return [(y, x) for y in sorted({0, H // 2, H - 1}) for x in range(W)]
    if kind == "corner":
        return [(y, x) for y in sorted({0, min(1, H - 1), H - 1}) for x in sorted({0, min(1, W - 1), W - 1})]
    if kind == "band_edge":     # the rows on both sides of the band boundaries (bands of 8 and 16 rows, the split layout's first four)
        rows = [r for r in (3, 4, 7, 8, 15, 16, H - 5, H - 4) if 0 <= r < H]
        return [(y, x) for y in rows for x in range(0, W, 3)]
    if kind == "self_tap":      # border pixels that are not corners: the clamp folds their outward taps onto the pixel itself
        px = [(0, x) for x in range(1, W - 1, 2)] + [(H - 1, x) for x in range(1, W - 1, 2)]
        px += [(y, 0) for y in range(1, H - 1, 2)] + [(y, W - 1) for y in range(1, H - 1, 2)]
        return px or [(0, 0)]
    raise ValueError(kind)


def make_inputs(family, W, H, seed=0):
    rng = np.random.default_rng([seed, W, H, FAMILIES.index(family)])
    d = _base(W, H, rng)
    if family == "tame":
        d["nrm"][0, 0] = 0
    elif family == "sky_none":
        d["sky"][:] = 0
    elif family == "sky_all":
        d["sky"][:] = 1
    elif family == "sky_checker":
        yy, xx = np.mgrid[0:H, 0:W]
        d["sky"] = ((yy + xx) & 1).astype(np.uint8)
    elif family == "sky_single_nonsky":
        d["sky"][:] = 1
        d["sky"][H // 2, W // 2] = 0
    elif family == "sky_band_rows":
        d["sky"][:] = 0
        for r in (7, 8, 15, 16):
            if r < H: d["sky"][r, :] = 1
        if H > 9: d["sky"][9, ::2] = 1
    elif family in ("constant", "constant_one_changed"):
        d["hdr"][:] = np.array([0.5, 0.25, 0.125], f32)
        d["alb"][:] = np.array([0.75, 0.5, 0.25], f32)
        d["nrm"][:] = np.array([0.0, 1.0, 0.0], f32)
        d["dep"][:] = f32(4.0)
        d["sky"][:] = 0
        if family == "constant_one_changed":          # one lane per wavefront breaks the all-distances-zero shortcut, in every term
            for y in range(0, H, 2):
                for x in range(y % 5, W, 29):
                    d["hdr"][y, x, 1] = f32(0.375); d["alb"][y, x, 0] = f32(0.5); d["dep"][y, x] = f32(4.5)
                    d["nrm"][y, x] = np.array([0.6, 0.8, 0.0], f32)
    elif family == "phi_zero":
        d["phi"] = (0.0, 0.0, 0.0, 0.0)
    elif family == "phi_negative":
        d["phi"] = (-3.0, -0.35, -2.0, -0.2)
    elif family == "phi_tiny":
        d["phi"] = (1e-6, 1e-6, 1e-6, 1e-6)
    elif family == "normals_zero":
        d["nrm"][:] = 0
        d["nrm"][::3, ::2] = np.array([-0.0, 0.0, -0.0], f32)
    elif family == "normals_nonunit":
        d["nrm"] = (d["nrm"] * rng.choice([f32(1e-3), f32(7.0), f32(1e6), f32(1e-18)], size=(H, W, 1))).astype(f32)
    elif family == "normals_overflow":          # components whose squares overflow binary32 (and some whose squares vanish)
        big = rng.choice([f32(1e20), f32(-3e19), f32(2e38), f32(1e-30)], size=(H, W, 3)).astype(f32)
        m = rng.uniform(size=(H, W, 1)) < 0.5
        d["nrm"] = np.where(m, big, d["nrm"]).astype(f32)
    elif family == "depth_inf":
        d["dep"][rng.uniform(size=(H, W)) < 0.3] = f32(np.inf)
        d["dep"][0, :] = f32(np.inf)
    elif family == "depth_equal":
        d["dep"][:] = f32(2.5)
    elif family == "all_dark":          # every luminance <= 0: cnt = 0, target = aeExposure
        d["hdr"] = -np.abs(d["hdr"])
        d["hdr"][::2, ::2] = 0
        d["hdr"][1::2, ::3] = f32(-0.0)
        d["sky"][:] = 0
    else:
        values, place = family.split("_", 1)
        specials = FINITE_SPECIALS if values == "finite" else NONFINITE_SPECIALS + FINITE_SPECIALS[:4]
        d["sky"][rng.uniform(size=(H, W)) < 0.5] = 0          # (mostly surface: sky pixels are only copied)
        for k, (y, x) in enumerate(_places(place, W, H, rng)):
            v = specials[k % len(specials)]
            what = (k // len(specials)) % 4
            if what == 0: d["hdr"][y, x, k % 3] = v
            elif what == 1: d["hdr"][y, x, :] = v
            elif what == 2: d["alb"][y, x, (k + 1) % 3] = v
            else: d["hdr"][y, x, (k + 2) % 3] = v; d["alb"][y, x, :] = v
    for k in ("hdr", "alb", "nrm", "dep"):
        d[k] = np.ascontiguousarray(d[k], dtype=f32)
    d["sky"] = np.ascontiguousarray(d["sky"], dtype=np.uint8)
    return d


def nan_aware_mismatches(a, b):
    """elements that differ bit for bit, every NaN counting as equal to every other NaN"""
    a = np.ascontiguousarray(a, dtype=f32); b = np.ascontiguousarray(b, dtype=f32)
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    return int(np.count_nonzero(na != nb) + np.count_nonzero((a.view(np.uint32) != b.view(np.uint32)) & ~na & ~nb))


def same_f32(a, b):
    a, b = f32(a), f32(b)
    return bool((np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32))


# ---- log terms for the exposure sum alone (0 = a skipped sample) ----------------------------------------------------------------------------------
EXPOSURE_LENGTHS = (1, 3, 511, 512, 513, 1023, 8191, 8192, 8193, 524287, 524288, 524289, 1300003)
EXPOSURE_FAMILIES = (
    "bright", "dark", "zero_chunks", "all_zero", "dyadic_even", "dyadic_odd", "hover_1024", "hover_2m12", "hover_zero", "below_2m12", "denormal",
    "inf_first", "inf_mid", "inf_last", "ninf_first", "ninf_mid", "ninf_last", "nan_first", "nan_mid", "nan_last", "huge_first", "huge_mid", "huge_last",
)
EXPOSURE_TAME = ("bright", "dark", "zero_chunks")


def exposure_terms(family, n, seed=0):
    rng = np.random.default_rng([seed, n, EXPOSURE_FAMILIES.index(family)])
    dark = lambda: np.log(f32(1e-6) + rng.random(n).astype(f32) ** f32(3)).astype(f32)
    if family == "bright":
        t = np.log(f32(1e-6) + rng.uniform(1.5, 50.0, n).astype(f32)).astype(f32)
    elif family == "dark":
        t = dark()
    elif family == "zero_chunks":          # whole chunks (512) and whole groups (8192) of zeros at the start, inside and at the end
        t = dark()
        t[rng.random(n) < 0.2] = 0
        for lo, hi in ((0, 512), (0, 8192 if n > 40000 else 0), (n // 2 // 512 * 512, n // 2 // 512 * 512 + 1024),
                       (n // 3 // 8192 * 8192, n // 3 // 8192 * 8192 + (16384 if n > 40000 else 0)), (max(0, (n - 1) // 512 * 512 - 8192), n)):
            t[lo:hi] = 0
        if n < 600: t[n // 2] = f32(-1.25)
    elif family == "all_zero":
        t = np.zeros(n, f32); t[::7] = f32(-0.0)
    elif family in ("dyadic_even", "dyadic_odd"):          # multiples of 2^-12 of both signs: half of them tie exactly at the sum's ulp of 2^-11, more later
        t = (rng.integers(-300, 700, n) / f32(4096.0)).astype(f32)
        t[0] = f32(4096.0) + (f32(2.0 ** -11) if family == "dyadic_odd" else f32(0))          # ulp 2^-11 from the start; the mantissa's parity set
    elif family == "hover_1024":
        t = rng.uniform(-0.02, 0.02, n).astype(f32); t[0] = f32(1024.0)
    elif family == "hover_2m12":
        t = (rng.uniform(-1.0, 1.0, n) * 2.0 ** -17).astype(f32); t[0] = f32(2.0 ** -12)
    elif family == "hover_zero":
        t = rng.uniform(-1.0, 1.0, n).astype(f32)
        t[1::2] = -t[0:(n // 2) * 2:2] * f32(1.0 + 2.0 ** -20)
    elif family == "below_2m12":
        t = (rng.uniform(0.0, 1.0, n) * 1e-10).astype(f32)
    elif family == "denormal":
        t = (rng.integers(-2000, 2000, n).astype(np.int64)).astype(f32) * f32(1.4e-45)
        t[rng.random(n) < 0.1] = 0
    else:
        what, where = family.split("_")
        t = dark()
        v = {"inf": f32(np.inf), "ninf": f32(-np.inf), "nan": f32(np.nan), "huge": f32(1e30)}[what]
        n_chunks = (n + 511) // 512
        at = {"first": min(3, n - 1), "mid": min(n - 1, ((n_chunks // 2) // 16 * 16 + 8) * 512 + 77), "last": max(0, n - 2 if n > 1 else 0)}[where]
        t[at] = v
    return np.ascontiguousarray(t, dtype=f32)


def serial_sum_f32(terms):
    """logSum += term, one binary32 addition after the other (numpy's cumulative sum is that loop)"""
    with np.errstate(all="ignore"):          # (from +0.0, as the loop: 0.0f + -0.0f is +0.0f)
        return np.cumsum(np.concatenate([np.zeros(1, f32), np.ascontiguousarray(terms, dtype=f32).ravel()]), dtype=f32)[-1]
