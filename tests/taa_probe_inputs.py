"""Inputs for TemporalBlendWithClamp (step 5 of TryFlipAndBlit) that no traced frame produces, drawn by seed: shared by the CPU test that holds
the oracle's temporal_blend to its Python restatement and carries the coverage conditions (test_taa_probe_cpu.py) and by the GPU test that holds
the TAA kernels to the oracle (test_gpu_taa_probe.py).  Every family returns the eight planes of a W x H trace grid as a dict -
cur, nrm (H, W, 3), dep (H, W), sky (H, W) u8 of this frame; hist, pnrm, pdep, psky of the frame before - in the argument order of
RaytraceRenderer.taa_probe / oracle_binding.taa_probe (`planes`).  Sky bytes are 0 or 1 only: k_gather_halo turns the flag into 1.0 / 0.0, other
bytes are outside what the kernel forms agree on.

Threshold pairs are FOUND, not computed: candidates are drawn around the threshold, the kernel's expression is evaluated on them in numpy's
binary32 (one correctly rounded operation at a time, the order of csrc/ycge_kernels.hip: taa_blend) and those that land on the wanted value
bit for bit are kept."""
import numpy as np

import py_restatement as pr

f32 = np.float32
FLT_MAX = np.finfo(f32).max
NAN, INF = f32(np.nan), f32(np.inf)

FAMILIES = ("tame", "thresholds", "nonfinite_depth", "normals", "sky_edges", "luminance", "nan_colours")
# families whose outputs may hold NaN (at most half of the history values: a NaN compares equal to any NaN)
NAN_FAMILIES = ("nonfinite_depth", "normals", "luminance", "nan_colours")
PLANE_KEYS = ("cur", "nrm", "dep", "sky", "hist", "pnrm", "pdep", "psky")
# the branches (py_restatement.temporal_blend's report) a family is named for: at least 32 pixels each at 40 x 40, default parameters
FAMILY_BRANCHES = {
    "tame": [("alpha", a) for a in range(5)] + [("clamp", k) for k in range(3)],
    "thresholds": [("alpha", pr.TAA_ALPHA_REL), ("alpha", pr.TAA_ALPHA_NDOT), ("alpha", pr.TAA_ALPHA_KEPT)],
    "nonfinite_depth": [("alpha", pr.TAA_ALPHA_DEPTH_NONFINITE), ("alpha", pr.TAA_ALPHA_REL), ("alpha", pr.TAA_ALPHA_KEPT)],
    "normals": [("alpha", pr.TAA_ALPHA_NDOT), ("alpha", pr.TAA_ALPHA_KEPT)],
    "sky_edges": [("alpha", pr.TAA_ALPHA_SKY), ("alpha", pr.TAA_ALPHA_KEPT)],
    "luminance": [("clamp", pr.TAA_CLAMP_ABOVE), ("clamp", pr.TAA_CLAMP_BELOW), ("clamp", pr.TAA_CLAMP_NONE)],
    "nan_colours": [("clamp", pr.TAA_CLAMP_NONE)],
}

# the raw config values walked over the families (the tile forms take radius 0 and 1 only)
ALPHAS = (-0.5, 0.0, 0.01, 0.5, 1.0, 3.0)
RADII = (0, 1, 2, 3)
PADS = (-0.25, 0.0, 0.1, 1.5)


def walk(k, tile_form=False):
    """the k-th parameter set (alpha, radius, pad): the three lists turn at different rates, 48 steps bring every radius x pad pair"""
    radii = RADII[:2] if tile_form else RADII
    return ALPHAS[k % len(ALPHAS)], radii[k % len(radii)], PADS[(k // 4 + k) % len(PADS)]


def family_walk(family, k, tile_form=False):
    """the k-th parameter set of a family: families start 7 steps apart (7 shares no factor with the 6 alphas, the 4 radii or the 2 radii of
    the tile forms), so at any one k - a shape, say - the families meet different alphas and different radii"""
    return walk(7 * FAMILIES.index(family) + k, tile_form)


def tile_cases(family, rank):
    """(reset, alpha, radius, pad) of the tile forms' calls for a family on a rank: ALWAYS one blend at radius 1 - the only radius at which a
    tap leaves the rank's tiles and a halo record is read - and one call at radius 0, a reset on every other (family, rank); alpha and pad
    move with the family and with the rank"""
    fi = FAMILIES.index(family)
    a1, _, p1 = walk(7 * fi + rank)
    a0, _, p0 = walk(7 * fi + rank + 3)
    return [(0, a1, 1, p1), ((fi + rank) % 2, a0, 0, p0)]


def planes(d):
    return [d[k] for k in PLANE_KEYS]


def nan_aware_mismatches(a, b):
    """elements that differ bit for bit, every NaN counting as equal to every other NaN (uint8 planes: plain differences)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype != f32:
        return int(np.count_nonzero(a != b))
    na, nb = np.isnan(a), np.isnan(b)
    return int(np.count_nonzero(na != nb) + np.count_nonzero((a.view(np.uint32) != b.view(np.uint32)) & ~na & ~nb))


# ---- the kernel's expressions in numpy binary32 ---------------------------------------------------------------------------------------------
def rel_f32(zn, zp):
    """dz / max(1e-4, min(z_now, z_prev)) on finite arrays without NaN"""
    zn, zp = np.asarray(zn, f32), np.asarray(zp, f32)
    with np.errstate(all="ignore"):
        return (np.abs(zn - zp) / np.maximum(f32(1e-4), np.minimum(zn, zp))).astype(f32)


def normalized_f32(v):
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        ls = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        inv = f32(1.0) / np.sqrt(ls)
        out = v * inv[..., None]
    return np.where((ls <= 0)[..., None], v, out).astype(f32)


def ndot_f32(a, b):
    a, b = normalized_f32(a), normalized_f32(b)
    with np.errstate(all="ignore"):
        return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(f32)


def luma_f32(c):
    c = np.asarray(c, f32)
    with np.errstate(all="ignore"):
        return ((f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]).astype(f32)


def _neighbours(t):
    t = f32(t)
    return [np.nextafter(t, f32(-np.inf)), t, np.nextafter(t, f32(np.inf))]


def depth_pairs_at_threshold(rng, per_target=16):
    """(z_now, z_prev) pairs whose rel is 0.05's lower neighbour, 0.05 and its upper neighbour, in that order, both orders of the two depths"""
    out = []
    for t in _neighbours(0.05):
        found = np.zeros((0, 2), f32)
        while len(found) < per_target:
            lo = rng.uniform(0.5, 40.0, 40000).astype(f32)
            hi = (lo * (f32(1.0) + t)).astype(f32)
            for k in range(-3, 4):          # (the rounding of lo * (1 + t) and of the division move the quotient by a few of its ulps)
                h = hi.copy()
                for _ in range(abs(k)):
                    h = np.nextafter(h, f32(np.inf) if k > 0 else f32(-np.inf))
                ok = rel_f32(h, lo) == t
                found = np.concatenate([found, np.stack([h[ok], lo[ok]], 1)])
        found = found[:per_target]
        found[1::2] = found[1::2, ::-1]          # every other pair the other way round: min() picks its second argument
        out.append(found)
    return out


def normal_pairs_at_threshold(rng, per_target=16):
    """(n_now, n_prev) pairs, neither of unit length, whose normalised dot is 0.8's lower neighbour, 0.8 and its upper neighbour"""
    out = []
    axes = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1]], f32)
    for t in _neighbours(0.8):
        found_a, found_b = np.zeros((0, 3), f32), np.zeros((0, 3), f32)
        while len(found_a) < per_target:
            n = 40000
            pick = rng.integers(0, 4, n)
            a = (axes[pick] * rng.choice([f32(0.25), f32(1.0), f32(3.0), f32(1e-3), f32(1e4)], (n, 1))).astype(f32)
            s = rng.uniform(0.1, 20.0, (n, 1)).astype(f32)
            along = f32(0.8) * (1 + rng.uniform(-2e-6, 2e-6, (n, 1))) * np.sign(a.sum(1, keepdims=True))
            across = f32(0.6) * (1 + rng.uniform(-2e-6, 2e-6, (n, 1)))
            b = np.zeros((n, 3))
            axis = np.argmax(np.abs(a), 1)
            b[np.arange(n), axis] = along[:, 0]
            b[np.arange(n), (axis + 1) % 3] = across[:, 0]
            b = (b * s).astype(f32)
            ok = ndot_f32(a, b) == t
            found_a, found_b = np.concatenate([found_a, a[ok]]), np.concatenate([found_b, b[ok]])
        out.append((found_a[:per_target], found_b[:per_target]))
    return out


# ---- the baseline ------------------------------------------------------------------------------------------------------------------------------
def _smooth(W, H, rng, lo, hi):
    """a low-frequency field with a little noise on it: neighbouring values are close, as in a picture"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ph = rng.uniform(0, 6.28, 4)
    f = 0.5 + 0.25 * np.sin(xx / 7.0 + ph[0]) * np.cos(yy / 5.0 + ph[1]) + 0.2 * np.sin((xx + yy) / 11.0 + ph[2]) + rng.uniform(-0.03, 0.03, (H, W))
    return (lo + (hi - lo) * np.clip(f, 0, 1)).astype(f32)


def _base(W, H, rng):
    """frame-like values: unit normals, positive depths (infinite on the sky, whose colour is a gradient), a history that is a running mean
    of nearly the same picture, sky in one connected region that moved by a row since the frame before"""
    cur = np.stack([_smooth(W, H, rng, 0.05, 2.5) for _ in range(3)], -1)
    nrm = rng.normal(size=(H, W, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(f32)
    dep = _smooth(W, H, rng, 1.0, 9.0)
    yy, xx = np.mgrid[0:H, 0:W]
    horizon = H * 0.3 + 2.0 * np.sin(xx / 6.0)
    sky = (yy < horizon).astype(np.uint8)
    psky = (yy < horizon + 1).astype(np.uint8)
    # the frame before: the same picture a little off - depths within a few per cent (some beyond 5), normals turned a little (some beyond acos 0.8)
    pdep = (dep * (1 + rng.choice([0.0, 0.01, -0.02, 0.04, 0.08, -0.09], (H, W), p=[0.3, 0.2, 0.2, 0.1, 0.1, 0.1]))).astype(f32)
    turn = rng.choice([0.0, 0.1, 0.3, 0.9, 1.5], (H, W, 1), p=[0.3, 0.2, 0.2, 0.15, 0.15])
    pn = nrm + turn * rng.normal(size=(H, W, 3))
    pnrm = (pn / np.linalg.norm(pn, axis=-1, keepdims=True)).astype(f32)
    hist = (cur * rng.choice([0.6, 0.9, 1.0, 1.1, 1.6], (H, W, 1), p=[0.2, 0.2, 0.2, 0.2, 0.2])).astype(f32)
    for s, z in ((sky, dep), (psky, pdep)):
        z[s == 1] = INF
    cur[sky == 1] = np.stack([0.3 + 0.4 * yy / max(1, H), 0.5 + 0.3 * yy / max(1, H), 0.9 + 0.0 * yy], -1).astype(f32)[sky == 1]
    return dict(cur=cur, nrm=nrm, dep=dep, sky=sky, hist=hist, pnrm=pnrm, pdep=pdep, psky=psky)


def _surface(d):
    """no sky at all, depths and normals that keep the configured alpha: what a family then changes is what decides"""
    d["sky"][:] = 0; d["psky"][:] = 0
    bad = ~np.isfinite(d["dep"])
    d["dep"][bad] = f32(3.0)
    d["pdep"] = d["dep"].copy()
    d["pnrm"] = d["nrm"].copy()


def _cells(W, H, rng, n_kinds, density=0.5):
    """kind per pixel: -1 = left alone, else 0 .. n_kinds - 1 in turn over a scattered `density` of the pixels (a pixel list in scan order)"""
    kind = np.full(W * H, -1, np.int64)
    at = np.flatnonzero(rng.uniform(size=W * H) < density)
    if len(at) == 0:
        at = np.array([0])
    kind[at] = np.arange(len(at)) % n_kinds
    return kind.reshape(H, W)


def make_inputs(family, W, H, seed=0):
    rng = np.random.default_rng([seed, W, H, FAMILIES.index(family)])
    d = _base(W, H, rng)
    if family == "tame":
        pass
    elif family == "thresholds":
        _surface(d)
        dp, npairs = depth_pairs_at_threshold(rng), normal_pairs_at_threshold(rng)
        floor = f32(1e-4)
        # min(z_now, z_prev) at, just under and far under the 1e-4 floor, zero, -0 and negative; the other depth a few 1e-6 away, so that
        # rel = dz / 1e-4 falls on both sides of 0.05
        mins = [floor, np.nextafter(floor, f32(0)), np.nextafter(floor, f32(1)), f32(1e-7), f32(1e-30), f32(1e-42), f32(0.0), f32(-0.0), f32(-1e-6), f32(-2.0)]
        dzs = [f32(4e-6), f32(5e-6), np.nextafter(f32(5e-6), f32(1)), f32(6e-6), f32(0.0), f32(1e-4)]
        kind = _cells(W, H, rng, 9, 0.7)
        for n, (y, x) in enumerate(zip(*np.nonzero(kind >= 0))):
            k, j = int(kind[y, x]), n // 9
            if k < 3:
                d["dep"][y, x], d["pdep"][y, x] = dp[k][j % len(dp[k])]
            elif k < 6:
                a, b = npairs[k - 3]
                d["nrm"][y, x], d["pnrm"][y, x] = (a[j % len(a)], b[j % len(a)]) if j % 2 else (b[j % len(a)], a[j % len(a)])
            else:
                m, dz = mins[j % len(mins)], dzs[(j // len(mins) + j) % len(dzs)]
                other = f32(m + dz) if m > 0 else dz          # (from zero and below: the other depth is dz itself, the floor divides)
                d["dep"][y, x], d["pdep"][y, x] = (m, other) if j % 2 else (other, m)
    elif family == "nonfinite_depth":
        _surface(d)
        specials = [INF, -INF, NAN, FLT_MAX, -FLT_MAX]
        kind = _cells(W, H, rng, 3, 0.6)
        for n, (y, x) in enumerate(zip(*np.nonzero(kind >= 0))):
            k, v = int(kind[y, x]), specials[(n // 3) % len(specials)]
            if k == 0: d["dep"][y, x] = v
            elif k == 1: d["pdep"][y, x] = v
            else: d["dep"][y, x] = v; d["pdep"][y, x] = specials[(n // 15 + n // 3) % len(specials)]
    elif family == "normals":
        _surface(d)
        scales = [f32(s) for s in (1e-23, 1e-22, 1e-21, 1e-20, 1e-19, 1e-10, 1e10, 1e18, 1e19, 3e19)]
        kind = _cells(W, H, rng, 8, 0.7)
        for n, (y, x) in enumerate(zip(*np.nonzero(kind >= 0))):
            k, j = int(kind[y, x]), n // 8
            if k == 0: d["nrm"][y, x] = 0                                          # zero on one side ...
            elif k == 1: d["pnrm"][y, x] = [0.0, -0.0, 0.0]
            elif k == 2: d["nrm"][y, x] = 0; d["pnrm"][y, x] = 0                   # ... and on both
            elif k == 3: d["nrm"][y, x] *= scales[j % len(scales)]                 # squared length denormal, zero or infinite
            elif k == 4: d["pnrm"][y, x] *= scales[j % len(scales)]
            elif k == 5: d["nrm"][y, x] *= scales[j % len(scales)]; d["pnrm"][y, x] *= scales[(j // len(scales)) % len(scales)]
            elif k == 6: (d["nrm"] if j % 2 else d["pnrm"])[y, x, j % 3] = [NAN, INF, -INF][(j // 3) % 3]
            else: (d["nrm"] if j % 2 else d["pnrm"])[y, x] = np.array([3e-41, -1e-42, 2e-40], f32) * f32(1 + j % 5)      # denormal components
    elif family == "sky_edges":
        yy, xx = np.mgrid[0:H, 0:W]
        band, col = yy * 4 // max(H, 1), xx * 2 // max(W, 1)
        sky = np.zeros((H, W), np.uint8)
        sky[(band == 0) & (col == 0)] = ((yy + xx) & 1)[(band == 0) & (col == 0)]                                   # a checkerboard
        sky[(band == 0) & (col == 1) & (yy % 4 == 1) & (xx % 4 == 1)] = 1                                            # single pixels
        sky[(band == 1) & (col == 0) & (yy % 3 == 1)] = 1                                                              # one-pixel stripes, lying
        sky[(band == 1) & (col == 1) & (xx % 3 == 1)] = 1                                                              # ... and standing
        sky[(band == 2) & (col == 0) & (yy % 4 == 1) & (xx % 5 < 2)] = 1                                             # pairs
        sky[(band == 2) & (col == 1) & (yy % 4 < 2) & (xx % 5 < 2)] = 1                                              # 2 x 2 blocks
        sky[(band == 3) & (col == 0) & (yy % 4 < 2) & (xx % 5 < 2) & ~((yy % 4 == 1) & (xx % 5 == 1))] = 1          # corners of three
        sky[[0, H - 1], :] = 1; sky[:, [0, W - 1]] = 1                                                                 # a solid border ...
        if H > 4 and W > 4:
            sky[H - 2, W // 2:] = 1; sky[1, 1] = 0; sky[0, W // 3] = 0; sky[H // 2, 0] = 0                             # ... two deep here, nicked there
        d["sky"] = sky
        d["psky"] = np.where(rng.uniform(size=(H, W)) < 1 / 3, 1 - sky, sky).astype(np.uint8)
        for s, z in ((d["sky"], d["dep"]), (d["psky"], d["pdep"])):
            z[:] = np.where(s == 1, INF, np.where(np.isfinite(z), z, f32(3.0)))
    elif family == "luminance":
        _surface(d)
        yy, xx = np.mgrid[0:H, 0:W]
        flat = (yy // 4 + xx // 4) % 3 == 0                      # 4 x 4 blocks of one constant colour: windows of range 0 inside them
        d["cur"][flat] = np.array([0.5, 0.25, 0.125], f32)
        neg = (yy // 4 + xx // 4) % 3 == 1                       # ... and blocks of negative colours
        d["cur"][neg] = -d["cur"][neg]
        kind = _cells(W, H, rng, 8, 0.6)
        tiny = [f32(1e-7), f32(9.9e-7), f32(1e-30), f32(1e-42), np.nextafter(f32(1e-6), f32(0))]
        for n, (y, x) in enumerate(zip(*np.nonzero(kind >= 0))):
            k, j = int(kind[y, x]), n // 8
            if k == 0: d["hist"][y, x] = [0.0, -0.0, 0.0][j % 3]                                            # luminance exactly 0
            elif k == 1: d["hist"][y, x] = tiny[j % len(tiny)]                                              # in (0, 1e-6)
            elif k == 2: d["hist"][y, x] = -np.abs(d["hist"][y, x]) * f32([1.0, 1e-6, 1e20][j % 3])         # negative
            elif k == 3: d["hist"][y, x] = d["cur"][y, x]                                                   # the centre tap's: l_max itself where the window is flat
            elif k == 4: d["hist"][y, x] = [INF, -INF, FLT_MAX][j % 3]
            elif k == 5: d["hist"][y, x] = d["cur"][y, x] * f32([4.0, 0.1][j % 2])                          # plainly above, plainly below
            elif k == 6 and j % 4 == 0: d["cur"][y, x] = f32([3e38, -3e38, 2e38][(j // 4) % 3])             # the range, or range * pad, overflows
            elif k == 7 and j % 4 == 0: d["cur"][y, x, j % 3] = f32([3.3e38, -3.3e38][(j // 4) % 2])
    elif family == "nan_colours":
        specials = [NAN, INF, -INF, NAN]
        at = np.flatnonzero(rng.uniform(size=W * H) < 0.06)          # isolated taps ...
        for n, i in enumerate(at if len(at) else [0]):
            y, x = divmod(int(i), W)
            if n % 2: d["cur"][y, x] = specials[(n // 2) % 4]
            else: d["cur"][y, x, n % 3] = specials[(n // 2) % 4]
        for n, i in enumerate(np.flatnonzero(rng.uniform(size=W * H) < 0.01)):          # ... and runs of them: several taps of one window, the centre among them
            y, x = divmod(int(i), W)
            d["cur"][y:y + 2, x:x + 3, n % 3] = specials[n % 4]
    else:
        raise ValueError(family)
    for k in PLANE_KEYS:
        d[k] = np.ascontiguousarray(d[k], dtype=np.uint8 if k in ("sky", "psky") else f32)
    assert set(np.unique(d["sky"])) | set(np.unique(d["psky"])) <= {0, 1}
    return d
