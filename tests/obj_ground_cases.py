"""Inputs of the auto-ground tests (tests/test_obj_ground_cpu.py, tests/test_gpu_obj_ground.py) as OBJ text, with the arrays they were drawn
from.  `v` lines are written with %.9g: the parse gives back the drawn binary32 values (nine significant digits identify a binary32) and
every token stays inside the kernels' exact float domain (at most 15 digits, a decimal exponent within +-22) - every file but INF_POSITION,
whose 1e39 the kernels hand to the host parser.

CASES: name -> Case(text, pos float32 [nv, 3], faces int32 [nt, 3], device_parse).  Built on first use and kept (get()); want_of(): the restatement's answer, kept likewise.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "text pos faces device_parse")

WINNER_SIZES = (63, 64, 65, 255, 256, 257, 1025)
STRIP = 1 << 15


def obj_text(pos, faces, v_lines=None) -> bytes:
    """`v_lines`: the literal text of some vertices' lines, {index: "v ..."}"""
    out = []
    for i, p in enumerate(np.asarray(pos, np.float32).tolist()):
        out.append(v_lines[i] if v_lines and i in v_lines else "v %.9g %.9g %.9g" % tuple(p))
    for a, b, c in np.asarray(faces).tolist():
        out.append("f %d %d %d" % (a + 1, b + 1, c + 1))
    return ("\n".join(out) + "\n").encode()


def case(pos, faces, **kw):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    return Case(obj_text(pos, faces, **kw), pos, faces, True)


def strip_faces(vertices):
    """a triangle strip along `vertices` (len - 2 faces, in order): one component"""
    v = np.asarray(vertices, np.int64)
    return np.stack([v[:-2], v[1:-1], v[2:]], axis=1)


def draw(rng, n, lo=-2.0, hi=2.0):
    return rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)


def _tie(rng):
    # two components of two faces each; the one whose faces come FIRST uses the HIGHER vertex indices
    pos = draw(rng, 8)
    return case(pos, [(4, 5, 6), (5, 6, 7), (0, 1, 2), (1, 2, 3)])


def _counts_1_2_2(rng):
    pos = draw(rng, 11)
    return case(pos, [(0, 1, 2), (3, 4, 5), (4, 5, 6), (7, 8, 9), (8, 9, 10)])


def _bridged(rng):
    # patches P (0..4) and Q (5..9) of three faces each, R (10..15) of four; only the LAST face joins P and Q: 7 faces against 4
    pos = draw(rng, 16)
    p = strip_faces(range(0, 5)).tolist()
    q = strip_faces(range(5, 10)).tolist()
    r = strip_faces(range(10, 16)).tolist()
    return case(pos, p + q + r + [(4, 2, 5)])


def _bow_tie(rng):
    # two fans of four faces around the shared vertex 0, and a strip of five faces beside them: 8 against 5
    pos = draw(rng, 18)
    fan_a = [(0, i, i + 1) for i in range(1, 5)]
    fan_b = [(0, i, i + 1) for i in range(6, 10)]
    return case(pos, strip_faces(range(11, 18)).tolist() + fan_a + fan_b)


def _degenerate_and_duplicate(rng):
    # A: (0, 1, 2) three times and the degenerate (0, 0, 0): 4 faces; B: two faces; a degenerate face alone on vertex 7
    pos = draw(rng, 8)
    return case(pos, [(7, 7, 7), (3, 4, 5), (0, 1, 2), (4, 5, 6), (0, 1, 2), (0, 0, 0), (0, 1, 2)])


def _outside(rng):
    # the winner lives in [-1, 1]^3; vertices no face names and the losing component's vertices lie far outside it
    win = draw(rng, 12, -1.0, 1.0)
    unnamed = draw(rng, 3, 900.0, 1000.0)
    lose = draw(rng, 4, -1000.0, -900.0)
    pos = np.vstack([unnamed[:2], lose, win, unnamed[2:]])
    return case(pos, strip_faces(range(2, 6)).tolist() + strip_faces(range(6, 18)).tolist())


def _winner(rng, n):
    # a loser of two faces FIRST in the file, then a strip of n faces
    pos = draw(rng, 4 + n + 2)
    return case(pos, strip_faces(range(0, 4)).tolist() + strip_faces(range(4, 4 + n + 2)).tolist())


def _strip(rng, order):
    n = STRIP + 2
    along = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "shuffled": rng.permutation(n)}[order]
    pos = np.empty((n, 3), np.float32)
    t = np.arange(n, dtype=np.float64)
    path = np.stack([t * 0.01, np.sin(t * 0.05), (t % 2) * 0.5], axis=1) + rng.uniform(-0.002, 0.002, size=(n, 3))
    pos[along] = path.astype(np.float32)
    return case(pos, strip_faces(along))


def _cancelling(rng):
    # offsets of about 1e3 of either sign with detail of about 1e-3: the running float32 sum rounds at every add, and differently from a tree
    n = 6000
    sign = rng.choice([-1.0, 1.0], size=(n, 3))
    pos = (sign * rng.uniform(500.0, 1500.0, size=(n, 3)) + rng.uniform(-1e-3, 1e-3, size=(n, 3))).astype(np.float32)
    return case(pos, strip_faces(range(n)))


def _y_zero(rng):
    # every y is a zero of either sign: the centroid's y is +0, the y extremes are -0 and +0
    pos = draw(rng, 10)
    pos[:, 1] = np.where(np.arange(10) % 3 == 0, np.float32(-0.0), np.float32(0.0))
    return case(pos, strip_faces(range(10)))


def _inf_position(rng):
    # 1e39 and -1e39 overflow to +inf and -inf: the kernels decline the tokens (exponent beyond 22), the host parser reads the file, and the x sum is inf + -inf
    pos = draw(rng, 9)
    pos[2, 0], pos[5, 0] = np.inf, -np.inf
    lines = {2: "v 1e39 %.9g %.9g" % (pos[2, 1], pos[2, 2]), 5: "v -1e39 %.9g %.9g" % (pos[5, 1], pos[5, 2])}
    c = case(pos, strip_faces(range(9)), v_lines=lines)
    return c._replace(device_parse=False)


def _grid(rng):
    # 257 x 257 vertices, 2^17 triangles, with islands of a few faces before, inside and behind the grid's faces
    w = 257
    ys, xs = np.mgrid[0:w, 0:w]
    height = rng.uniform(-0.05, 0.05, size=(w, w))
    grid = np.stack([xs * 0.01, height + 0.3 * np.sin(xs * 0.03) * np.cos(ys * 0.02), ys * 0.01], axis=2).reshape(-1, 3)
    i = (ys[:-1, :-1] * w + xs[:-1, :-1]).reshape(-1)
    quads = np.stack([np.stack([i, i + 1, i + w], axis=1), np.stack([i + 1, i + w + 1, i + w], axis=1)], axis=1).reshape(-1, 3)
    base = w * w
    islands = draw(rng, 15, 5.0, 9.0)
    pos = np.vstack([grid, islands])
    isl = [strip_faces(range(base + 5 * k, base + 5 * k + 5)) for k in range(3)]
    half = len(quads) // 2
    return case(pos, np.vstack([isl[0], quads[:half], isl[1], quads[half:], isl[2]]))


_BUILDERS = {
    "one_triangle": lambda rng: case(draw(rng, 3), [(0, 1, 2)]),
    "tie_first_has_higher_indices": _tie,
    "counts_1_2_2": _counts_1_2_2,
    "bridged_by_a_later_face": _bridged,
    "bow_tie": _bow_tie,
    "degenerate_and_duplicate": _degenerate_and_duplicate,
    "unnamed_and_losers_outside": _outside,
    "cancelling": _cancelling,
    "y_extreme_zero": _y_zero,
    "inf_position": _inf_position,
    "grid_with_islands": _grid,
}
_BUILDERS.update({f"winner_{n}": (lambda rng, n=n: _winner(rng, n)) for n in WINNER_SIZES})
_BUILDERS.update({f"strip_{o}": (lambda rng, o=o: _strip(rng, o)) for o in ("ascending", "descending", "shuffled")})

NAMES = tuple(sorted(_BUILDERS))
SMALL = tuple(n for n in NAMES if not n.startswith(("strip_", "grid_")))          # what a sanitized stand-alone program runs through
ZERO_EXTREME = ("y_extreme_zero",)                                                # where the sign convention of a zero extreme shows
NAN_CENTROID = ("inf_position",)                                                 # where mesh_loader's np.min / np.max hand a NaN on and the reference's compares do not
_built = {}


def get(name) -> Case:
    if name not in _built:
        _built[name] = _BUILDERS[name](np.random.default_rng([20261, NAMES.index(name)]))
    return _built[name]


_want = {}


def want_of(name) -> dict:
    """tests/obj_ground_restatement.py's answer for a case, computed once per process and shared by the tests that need it"""
    if name not in _want:
        import obj_ground_restatement
        c = get(name)
        _want[name] = obj_ground_restatement.ground(c.pos, c.faces)
    return _want[name]
