"""Scenes and rays for the seams of the scene walk (csrc/ycge_rt.hip.h): rays that start exactly in the plane of a box, pass exactly through an
edge two primitives share, end exactly at tMax, put a denominator next to its cut-off, or cross voxel cells at their edges and corners - the
decisions no ray drawn from a continuous distribution reaches.  numpy only.  Shared by the CPU test that holds the conditions of these inputs
(test_seam_rays_cpu.py: a class that never reaches its seam fails there) and by the GPU test that holds Scene.Hit / Scene.Occluded on the device
to the oracle on them (test_gpu_seam_rays.py).

Every coordinate, radius and voxel size of the three scenes is a multiple of 1/8 below 64, so sums and differences of them are exact in
binary32.  The query normalises the direction as `new Ray(o, d)` does (Ray.cs:8-12); exact constructions therefore use axis directions whose
length is a power of two (they normalise to +-1 with +-0 elsewhere, both zero signs are used) or the symmetric diagonals (+-1, 0, +-1) and
(+-1, +-1, +-1), whose components stay equal after normalisation.  Everything else is an *ulp fan*: d = target - o aimed at a seam point from an
origin off the lattice, emitted five times with the origin moved -2 .. +2 ulps along an axis perpendicular to the seam.

A ray class is a function that returns (rays[n, 8] float32 = {o, d, tmin, tmax}, labels[n]); at most 4 096 rays a class and scene."""
import itertools

import numpy as np

from yetanotherconsolegameengine_amd import scenes as _scenes
from yetanotherconsolegameengine_amd.scene import (AmbientLight, Box, CylinderY, Disk, Material, Mesh, Plane, PointLight, Scene, Sphere, Triangle,
                                                   VolumeGrid, XYRect, XZRect, YZRect, vec3)

F32 = np.float32
FLT_MAX = F32(3.4028234663852886e38)
INF = F32(np.inf)
MAX_RAYS = 4096
FAN = 5                                                         # rays of one fan: the origin moved -2 .. +2 ulps
SCENES = ("analytic", "mixed", "voxels")
CLASSES = ("slab_nan", "edge_tie", "interval_end", "threshold", "voxel_seam")
WIRE_FRAC = 0.125                                               # a dyadic wire_width_frac: wire_width_frac * voxel is exact


# --------------------------------------------------------------------------------------------------------------------------- scenes
def _mat(k):
    """a distinct dull albedo per object: the albedo of a record names its object"""
    return Material(vec3(0.2 + 0.05 * (k % 13), 0.25 + 0.04 * (k % 17), 0.3 + 0.03 * (k % 19)))


_WIDE_X = (0, 1, 2, 4, 5, 8, 9, 10, 12)                        # quarters: columns and rows of uneven width, so that the builder's leaves
_WIDE_Y = (0, 2, 3, 4, 5, 6, 9, 10, 11)                        # come out in different sizes (3 and 5 among the 8s)


def _bump(i, j):
    """0 .. 4 quarters towards the viewer"""
    return (i * i + 3 * j) % 5


def _lattice_mesh(x0, y0, z0, bumpy, twice):
    """8 x 8 quads, each split into two triangles along its (1, 0) - (0, 1) diagonal, vertices on multiples of 1/4.  bumpy: uneven columns and
    rows, vertices 0 .. 4 quarters nearer (a tree with several leaves of different sizes); otherwise level squares of side 1/4.
    twice: every quad a second time, so every t is a tie"""
    q = F32(0.25)
    xs, ys = (_WIDE_X, _WIDE_Y) if bumpy else (range(9), range(9))
    def v(i, j):
        return [F32(x0) + q * F32(xs[i]), F32(y0) + q * F32(ys[j]), F32(z0) + (q * F32(_bump(i, j)) if bumpy else F32(0))]
    tris = []
    for rep in range(2 if twice else 1):
        for j in range(8):
            for i in range(8):
                tris.append([v(i, j), v(i + 1, j), v(i, j + 1)])
                tris.append([v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)])
    return np.array(tris, F32)


def _cells(shape, seed, fill=0.5):
    rng = np.random.default_rng(seed)
    c = np.zeros(tuple(shape) + (2,), np.int32)
    c[..., 0] = np.where(rng.random(shape) < fill, rng.integers(1, 12, shape), 0)
    return c


def _analytic_objects():
    o = []
    add = lambda cls, *a: o.append((cls, a))
    add(Plane, vec3(0, 0, 0), vec3(0, 1, 0), 0.0, 0.0)
    for c, r in (((0, 2, -8), 1.25), ((0, 2, -8), 1.25), ((4, 2, -8), 0.625), ((0, 6, -8), 1.25), ((4, 6, -8), 1.25), ((-4, 6, -8), 1.25), ((-8, 6, -8), 0.625),
                 ((8, 6, -8), 1.25), ((-8, 2, -20), 1.25), ((-4, 2, -20), 0.625), ((0, 2, -20), 1.25), ((4, 2, -20), 1.25), ((8, 2, -20), 1.25)):
        add(Sphere, vec3(*c), r)                                # (the first one twice: a duplicated sphere; radii 5/8 and 5/4: 3 : 4 : 5 tangents are dyadic)
    for mn, mx in (((-8, 0, -8), (-6, 2, -6)), ((-6, 0, -8), (-4, 2, -6)), ((8, 0, -8), (10, 2, -6)), ((12, 1, -8), (13, 3, -7)), ((-12, 0, -8), (-10, 1, -7))):
        add(Box, vec3(*mn), vec3(*mx), 0.0, 0.0)                # (the first two share the face x = -6)
    add(Disk, vec3(9, 2, -7), vec3(0, 1, 0), 0.5, 0.0, 0.0)     # coplanar with the +Y face of the third box
    add(Disk, vec3(0, 1, -12), vec3(0, 1, 0), 1.25, 0.0, 0.0)
    add(Disk, vec3(4, 1, -12), vec3(1, 0, 1), 1.0, 0.0, 0.0)    # tilted
    add(Disk, vec3(-4, 1, -12), vec3(0, 0, 1), 1.0, 0.0, 0.0)   # upright: the radius test ignores y
    add(XYRect, 8.5, 9.5, 0.5, 1.5, -6.0, 0.0, 0.0)             # coplanar with the +Z face of the third box
    add(XYRect, 12.0, 14.0, 4.0, 6.0, -0.125, 0.0, 0.0)
    add(XZRect, 8.0, 10.0, -14.0, -12.0, 0.125, 0.0, 0.0)
    add(XZRect, -12.0, -10.0, -14.0, -12.0, 3.0, 0.0, 0.0)
    add(YZRect, 0.0, 2.0, -14.0, -12.0, 12.0, 0.0, 0.0)
    add(YZRect, 4.0, 6.0, -2.0, -1.0, 0.125, 0.0, 0.0)
    add(CylinderY, vec3(0, 0, -16), 1.0, 0.0, 2.0, True)
    add(CylinderY, vec3(4, 0, -16), 1.0, 0.0, 2.0, False)
    add(CylinderY, vec3(-4, 0, -16), 1.0, 0.125, 2.0, True)
    add(Triangle, vec3(8, 0, -16), vec3(10, 0, -16), vec3(8, 2, -16))          # two that share the edge (10, 0) - (8, 2)
    add(Triangle, vec3(10, 0, -16), vec3(10, 2, -16), vec3(8, 2, -16))
    for a, b in (((12, 0), (14, 0)), ((14, 0), (14, 2)), ((14, 2), (12, 2)), ((12, 2), (12, 0))):          # four that share the vertex (13, 1)
        add(Triangle, vec3(13, 1, -16), vec3(a[0], a[1], -16), vec3(b[0], b[1], -16))
    add(Triangle, vec3(-8, 0, -16), vec3(-6, 0, -16), vec3(-7, 2, -17))
    return o


def _cards():
    """four boxes of no thickness in the plane z = -28, apart from everything else: the builder gives them a leaf of their own, a node whose
    box has min.z == max.z.  For a ray in that plane with d.z == 0 BOTH slab products of the axis are 0 * inf: the one case in which a
    min / max that drops a NaN answers differently from MathF.Max / Min, which keep it (a NaN beside an infinity loses either way)."""
    return [(Box, (vec3(x, 10, -28), vec3(x + 1, 11, -28), 0.0, 0.0)) for x in (-4, -2, 1, 3)]


def _instantiate(specs):
    out = []
    for k, (cls, a) in enumerate(specs):
        m = _mat(k)
        if cls in (Sphere, Triangle):
            out.append(cls(*a, m))
        elif cls is CylinderY:
            out.append(cls(*a, m))
        elif cls is Plane:
            out.append(Plane(a[0], a[1], m, a[2], a[3]))
        elif cls is Disk:
            out.append(Disk(a[0], a[1], a[2], m, a[3], a[4]))
        elif cls is Box:
            out.append(Box(a[0], a[1], m, a[2], a[3]))
        else:
            out.append(cls(*a[:5], m, a[5], a[6]))
    return out


_SCENE_CACHE = {}


def scene(name):
    """one of SCENES (built once): the Scene the oracle and the library are both given"""
    if name in _SCENE_CACHE:
        return _SCENE_CACHE[name]
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.1)
    s.Lights.append(PointLight(vec3(2.0, 12.0, 4.0), vec3(1, 1, 1), 120.0))
    if name == "analytic":
        s.Objects = _instantiate(_analytic_objects() + _cards())
    elif name == "mixed":
        an = _instantiate(_analytic_objects())
        keep = [0, 1, 2, 3, 14, 15, 16, 19, 20, 29, 30, 32, 33, 34, 35, 36, 37]
        s.Objects = [an[k] for k in keep]
        s.Objects.append(Mesh(_lattice_mesh(1.0, 1.0, -24.0, True, False), _mat(50)))
        s.Objects.append(Mesh(_lattice_mesh(5.0, 1.0, -24.0, False, True), _mat(51)))
        s.Objects.append(VolumeGrid(_cells((8, 8, 8), 11), vec3(-8, 0, -32), vec3(1, 1, 1), _scenes.VoxelMaterialLookup, False, WIRE_FRAC, 16.0))
        s.Objects += _instantiate(_cards())
    elif name == "voxels":
        s.IsVolumeScene = True
        unit = vec3(1, 1, 1)
        for k, (cx, cz) in enumerate(((-8.125, -8.0), (-0.125, -8.0), (-8.125, 0.0), (-0.125, 0.0))):       # 2 x 2 chunks side by side, faces shared
            s.Objects.append(VolumeGrid(_cells((8, 8, 8), 20 + k), vec3(cx, 0, cz), unit, _scenes.VoxelMaterialLookup, k == 3, WIRE_FRAC, 16.0))
        s.Objects.append(VolumeGrid(_cells((8, 8, 8), 0, fill=0.0), vec3(7.875, 0, -8.0), unit, _scenes.VoxelMaterialLookup, False, WIRE_FRAC, 16.0))      # all air
        one = _cells((8, 8, 8), 0, fill=0.0); one[7, 0, 7, 0] = 3
        s.Objects.append(VolumeGrid(one, vec3(7.875, 0, 0.0), unit, _scenes.VoxelMaterialLookup, False, WIRE_FRAC, 16.0))                                  # one solid voxel in a corner
        s.Objects.append(VolumeGrid(_cells((9, 13, 17), 31), vec3(-16.125, 0.125, -3.875), vec3(0.25, 0.25, 0.25), _scenes.VoxelMaterialLookup, True, WIRE_FRAC, 16.0))
        s.Objects.append(VolumeGrid(_cells((8, 8, 8), 32), vec3(-8.125, 8, -8.0), unit, _scenes.VoxelMaterialLookup, False, WIRE_FRAC, 16.0))
        s.Objects.append(VolumeGrid(_cells((8, 8, 8), 33), vec3(-0.125, 8, 0.0), unit, _scenes.VoxelMaterialLookup, False, WIRE_FRAC, 16.0))
    else:
        raise KeyError(name)
    _SCENE_CACHE[name] = s
    return s


def of_type(s, cls):
    return [(i, o) for i, o in enumerate(s.Objects) if isinstance(o, cls)]


def solid_boxes(s):
    """the Box objects that have a volume (the cards of no thickness have no edge between two faces)"""
    return [(i, o) for i, o in of_type(s, Box) if all(a < b for a, b in zip(o.Min, o.Max))]


def kind_of(s, obj, sub):
    """the primitive kind of a hit: the object's class, a cylinder split into side and cap"""
    o = s.Objects[int(obj)]
    if isinstance(o, CylinderY):
        return "cylinder_side" if int(sub) == 0 else "cylinder_cap"
    return type(o).__name__


# --------------------------------------------------------------------------------------------------------------------------- helpers
def pack(o, d, tmin=0.0, tmax=FLT_MAX):
    o = np.atleast_2d(np.asarray(o, F32)); d = np.atleast_2d(np.asarray(d, F32))
    n = max(o.shape[0], d.shape[0])
    r = np.zeros((n, 8), F32)
    r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, F32(tmin), F32(tmax)
    return r


def normalized(d):
    """Vec3.Normalized (Vec3.cs:98-107) in binary32, rows of an array"""
    d = np.atleast_2d(np.asarray(d, F32))
    l2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F32(1.0) / np.sqrt(l2)).astype(F32)
    return np.where((l2 <= 0)[:, None], d, (d * inv[:, None]).astype(F32)).astype(F32)


def ulps(x, k):
    """x moved k binary32 values up (k < 0: down)"""
    x = np.array(x, F32)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf)).astype(F32)
    return x


def nudged(rays, axis, k):
    """the rays with each origin moved k ulps along its own axis (axis: one index per ray)"""
    out = np.array(rays, F32, copy=True)
    axis = np.broadcast_to(np.asarray(axis), (out.shape[0],))
    for a in range(3):
        m = axis == a
        out[m, a] = ulps(out[m, a], k)
    return out


def _cap(rays, labels, seed, group=1, extra=None):
    """at most MAX_RAYS rays, whole groups of `group` kept together, a seeded choice"""
    n = rays.shape[0] // group
    extra = extra or []
    if n * group > MAX_RAYS:
        sel = np.sort(np.random.default_rng(seed).choice(n, MAX_RAYS // group, replace=False))
        idx = (sel[:, None] * group + np.arange(group)[None, :]).ravel()
        return (rays[idx], labels[idx]) + tuple(e[idx] for e in extra)
    return (rays, labels) + tuple(extra)


def _cat(parts):
    """[(rays, label or labels, extra columns ...)] -> arrays"""
    rays = np.concatenate([p[0] for p in parts]).astype(F32)
    labels = np.concatenate([np.broadcast_to(np.asarray(p[1], dtype="U32"), (p[0].shape[0],)) for p in parts])
    extras = [np.concatenate([np.broadcast_to(np.asarray(p[2 + k]), (p[0].shape[0],)) for p in parts]) for k in range(len(parts[0]) - 2)]
    return (rays, labels) + tuple(extras)


def grid_box(g):
    """min / max of a VolumeGrid as VolumeGrid.cs:387-404 computes them"""
    n = np.asarray(g.Cells).shape[:3]
    mn = np.array(g.MinCorner, F32); sz = np.maximum(F32(1e-6), np.array(g.VoxelSize, F32))
    return mn, (mn + np.array(n, F32) * sz).astype(F32), sz


def solid_box(g, margin=1):
    """the box of the grid's solid voxels, `margin` voxels wider on every side (GGrid::solid_lo / solid_hi take one); None: no solid voxel"""
    mn, _, sz = grid_box(g)
    idx = np.argwhere(np.asarray(g.Cells)[..., 0] > 0)
    if idx.size == 0:
        return None
    lo, hi = idx.min(axis=0), idx.max(axis=0)
    return (mn + (lo - margin).astype(F32) * sz).astype(F32), (mn + (hi + 1 + margin).astype(F32) * sz).astype(F32)


def seam_boxes(name, oracle_renderer):
    """(m, 6) boxes whose planes slab_nan puts origins in: every node of the scene tree and of each mesh tree as the oracle built them (roots
    included), every grid's box, and each grid's solid-voxel box with and without the margin"""
    from yetanotherconsolegameengine_amd import abi
    s = scene(name)
    out = []
    nodes = oracle_renderer.accel(abi.ACCEL_SCENE_NODES)
    out += [np.concatenate([n["min"], n["max"]]) for n in nodes]
    for k in range(len(of_type(s, Mesh))):
        out += [np.concatenate([n["min"], n["max"]]) for n in oracle_renderer.accel(abi.ACCEL_MESH_NODES, k)]
    for _, g in of_type(s, VolumeGrid):
        mn, mx, _ = grid_box(g)
        out.append(np.concatenate([mn, mx]))
        for margin in (0, 1):
            sb = solid_box(g, margin)
            if sb is not None:
                out.append(np.concatenate(sb))
    b = np.array(out, F32).reshape(-1, 6)
    return b[(np.abs(b) < 1e5).all(axis=1)]                        # (a Plane's box is +-1e6: not a seam a ray is put on)


# --------------------------------------------------------------------------------------------------------------------------- slab_nan
def _rect_family(a0, a1, b0, b1, k, axis):
    """the rect-edge KAT's rays (test_oracle_kats.py:159-165) for one axis-aligned rectangle: straight at it, the origin exactly on each of its
    four edges and at a corner, the in-plane direction components +0 and -0"""
    ia, ib = [x for x in range(3) if x != axis]
    out = []
    for pa, pb in ((a0, 0.5 * (b0 + b1)), (a1, 0.5 * (b0 + b1)), (0.5 * (a0 + a1), b0), (0.5 * (a0 + a1), b1), (a0, b0), (a1, b1)):
        for side in (1.0, -1.0):
            for z in (0.0, -0.0):
                o = np.zeros(3, F32); d = np.full(3, z, F32)
                o[ia], o[ib], o[axis] = pa, pb, k + 2.0 * side
                d[axis] = -side
                out.append(np.concatenate([o, d]))
    return np.array(out, F32)


def slab_nan(name, boxes):
    """origins exactly in a plane of a box with a zero direction component on that axis: the slab product is 0 * inf = NaN, which BVH.BoxHitFast
    propagates (BVH.cs:228-235) and the hardware's max / min do not - the reason box_scene keeps two forms"""
    s = scene(name)
    parts = []
    dirs2 = ((1.0, 0.0), (-1.0, -0.0), (0.0, 2.0), (-0.0, -0.5), (1.0, 1.0), (-1.0, 1.0), (0.25, -0.75))       # axis, diagonal, generic, in the two other axes
    for bi, b in enumerate(boxes):
        lo, hi = b[:3], b[3:]
        cen = (F32(0.5) * (lo + hi)).astype(F32)
        for a in range(3):
            ia, ib = [x for x in range(3) if x != a]
            for plane in (lo[a], hi[a]):
                for where in ("in", "out"):
                    for z in (0.0, -0.0):
                        da, db = dirs2[(bi + a + (where == "in") + int(np.signbit(z)) * 3) % len(dirs2)]
                        o = cen.copy(); d = np.zeros(3, F32)
                        o[a] = plane
                        if where == "out":
                            o[ia] = hi[ia] + F32(1.0)
                        d[a], d[ia], d[ib] = z, da, db
                        o[ia] -= F32(4.0) * F32(da); o[ib] -= F32(4.0) * F32(db)          # back along the direction: the box lies ahead
                        parts.append((np.concatenate([o, d])[None, :], "box_plane"))
    fam = []
    for _, o in of_type(s, (XYRect, XZRect, YZRect)):
        if isinstance(o, XYRect): fam.append(_rect_family(o.X0, o.X1, o.Y0, o.Y1, o.Z, 2))
        elif isinstance(o, XZRect): fam.append(_rect_family(o.X0, o.X1, o.Z0, o.Z1, o.Y, 1))
        else: fam.append(_rect_family(o.Y0, o.Y1, o.Z0, o.Z1, o.X, 0))
    for _, o in of_type(s, Box):
        mn, mx = o.Min, o.Max
        for axis in range(3):
            ia, ib = [x for x in range(3) if x != axis]
            for k in (mn[axis], mx[axis]):
                fam.append(_rect_family(mn[ia], mx[ia], mn[ib], mx[ib], k, axis))
    for _, o in of_type(s, Disk):
        n = np.array(o.Normal, F32)
        if np.count_nonzero(n) == 1:                                # an axis-aligned disk: its bounding square's edges touch the rim
            axis = int(np.nonzero(n)[0][0]); c, r = o.Center, o.Radius
            ia, ib = [x for x in range(3) if x != axis]
            fam.append(_rect_family(c[ia] - r, c[ia] + r, c[ib] - r, c[ib] + r, c[axis], axis))
    r6 = np.concatenate([p[0] for p in parts] + fam).astype(F32) if (parts or fam) else np.zeros((0, 6), F32)
    labels = np.array(["box_plane"] * len(parts) + ["rect_edge"] * sum(f.shape[0] for f in fam), dtype="U32")
    rays = np.concatenate([r6, np.zeros((r6.shape[0], 1), F32), np.full((r6.shape[0], 1), FLT_MAX, F32)], axis=1)
    return _cap(rays, labels, 1)


def slab_event(rays, boxes):
    """per ray: some box has a plane with (plane - o) == 0 on an axis whose direction component is zero"""
    o, d = rays[:, 0:3], normalized(rays[:, 3:6])
    ev = np.zeros(rays.shape[0], bool)
    for a in range(3):
        on = (o[:, a][:, None] == boxes[:, a][None, :]) | (o[:, a][:, None] == boxes[:, 3 + a][None, :])
        ev |= on.any(axis=1) & (d[:, a] == 0)
    return ev


# --------------------------------------------------------------------------------------------------------------------------- edge_tie
def _box_edges(mn, mx):
    """(point, [outward normals of the faces that meet there]) for a point on each of the 12 edges and the 8 corners of a box; the edge points
    lie 3/8 off the middle, a coordinate no plane of the scenes has"""
    mn, mx = np.array(mn, F32), np.array(mx, F32)
    cen = F32(0.5) * (mn + mx) + F32(0.375)
    out = []
    for a, b in itertools.combinations(range(3), 2):
        for sa, sb in itertools.product((-1.0, 1.0), repeat=2):
            p = cen.copy(); p[a] = mx[a] if sa > 0 else mn[a]; p[b] = mx[b] if sb > 0 else mn[b]
            na, nb = np.zeros(3, F32), np.zeros(3, F32); na[a], nb[b] = sa, sb
            out.append((p, [na, nb]))
    for sg in itertools.product((-1.0, 1.0), repeat=3):
        p = np.where(np.array(sg) > 0, mx, mn).astype(F32)
        out.append((p, [np.eye(3, dtype=F32)[k] * F32(sg[k]) for k in range(3)]))
    return out


def _mesh_seams(tris):
    """((x, y, z), perpendicular axis, label) for seams of a lattice mesh seen along -z: its inner vertices, and the midpoints of the three kinds of edges"""
    v = tris.reshape(-1, 3)
    xs, ys = np.unique(v[:, 0]), np.unique(v[:, 1])
    z = {(float(p[0]), float(p[1])): F32(p[2]) for p in v}
    zv = lambda i, j: z[(float(xs[i]), float(ys[j]))]
    h = F32(0.5)
    out = []
    for j in range(9):
        for i in range(9):
            if 0 < i < 8 and 0 < j < 8:
                out.append(((xs[i], ys[j], zv(i, j)), 0, "mesh_vertex"))
            if i < 8 and 0 < j < 8:
                out.append(((h * (xs[i] + xs[i + 1]), ys[j], h * (zv(i, j) + zv(i + 1, j))), 1, "mesh_edge"))           # an edge along x
            if j < 8 and 0 < i < 8:
                out.append(((xs[i], h * (ys[j] + ys[j + 1]), h * (zv(i, j) + zv(i, j + 1))), 0, "mesh_edge"))           # an edge along y
            if i < 8 and j < 8:                                     # the diagonal two triangles of one quad share
                out.append(((h * (xs[i] + xs[i + 1]), h * (ys[j] + ys[j + 1]), h * (zv(i + 1, j) + zv(i, j + 1))), 0, "mesh_pair"))
    return out


def oracle_records(o, rays, brute=False):
    """(flag[n], rec[n, 13]) of an oracle renderer's scene_hit: {hit, object, sub, t, P, N, albedo} per ray; brute: the loop over all objects.
    The one function through which both test files get the oracle's answers to these rays."""
    rec = np.zeros((rays.shape[0], 13), F32)
    for i, r in enumerate(rays):
        rec[i] = o.scene_hit(r[0:3], r[3:6], r[6], r[7], brute=brute)
    return rec[:, 0] != 0, rec


def outcomes_of(rec):
    """(hit, object, sub) per record of the oracle: what a seam decides"""
    return [tuple(int(v) for v in r[0:3]) if r[0] != 0 else (0, -1, -1) for r in rec]


def edge_tie_exact(name):
    """(rays, labels, perp): rays exactly through a seam; perp: the axis along which an origin moved one ulp leaves the seam to either side.
    `exact:*` rays hit, and among the ray and its two neighbours along perp there are two outcomes (held by test_seam_rays_cpu.py for every
    one of them).  `tied:*` are ties in t alone - two surfaces in one plane - which no sideways step resolves.  `slab:*` are tangents that
    can only start in a plane of their object's own box, `blunt:*` edges whose one-ulp step is below a rounding: exact on paper, sent to
    the device like the rest, no condition claimed."""
    s = scene(name)
    parts = []

    def binade(v):
        return int(np.frexp(abs(float(v)))[1]) if v != 0 else -999

    def place(p, n, axes, kind):
        """the origin p + k n and the axis to step along.  A step of one ulp of o[a] is seen when that ulp is not below the rounding of
        anything it is added to or compared with: o[a] lies in a higher binade than the origin's other perpendicular coordinates and in no
        lower one than the seam point's.  The first distance k that gives such an axis is taken (`exact:`); an edge that has none at any
        of the distances keeps k = 2 and the widest axis and says so in its label (`blunt:`)."""
        for k in (2.0, 1.0, 4.0, 0.5, 3.0):
            o = (p + F32(k) * n).astype(F32)
            if o[1] <= 0.25:
                continue
            for a in axes:
                if all(binade(o[a]) > binade(o[b]) for b in axes if b != a) and all(binade(o[a]) >= binade(p[c]) for c in axes):
                    return pack(o, -n), "exact:" + kind, a
        o = (p + F32(2.0) * n).astype(F32)
        return pack(o, -n), "blunt:" + kind, max(axes, key=lambda a: abs(float(o[a])))

    for _, o in solid_boxes(s):
        for p, ns in _box_edges(o.Min, o.Max):
            if p[1] <= 0: continue                                  # (an edge that lies in the floor)
            n = np.sum(ns, axis=0).astype(F32)
            axes = [int(np.nonzero(v)[0][0]) for v in ns]
            parts.append(place(p, n, axes, "box_edge" if len(ns) == 2 else "box_corner"))       # into the box through the edge
            if len(ns) == 2:
                g = (ns[0] - ns[1]).astype(F32)                                                  # past the box, touching the edge only
                parts.append(place(p, g, axes, "box_graze"))
                parts.append(place(p, -g, axes, "box_graze"))
    boxes = solid_boxes(s)
    if len(boxes) >= 2:                                             # the face x = -6 two boxes share: from inside either, and along it
        parts.append((pack((-7, 1, -7), (2, 0, 0)), "tied:shared_face", 1))
        parts.append((pack((-5, 1, -7), (-1, -0.0, 0)), "tied:shared_face", 1))
        parts.append((pack((-7, 1, -7), (1, 0, -0.0), tmax=1.0), "tied:shared_face", 1))
        for z in (0.0, -0.0):
            parts.append((pack((-6, 1, -4), (z, 0, -1)), "exact:shared_face_edge", 0))
            parts.append((pack((-6, 4, -7), (z, -4, 0)), "exact:shared_face_edge", 0))
    for _, c in of_type(s, CylinderY):
        cx, cz, r = F32(c.Center[0]), F32(c.Center[2]), F32(c.Radius)
        for ycap, sy in ((F32(c.YMax), 1.0), (F32(c.YMin), -1.0)):
            if ycap <= 0: continue                                  # (a rim that lies in the floor)
            for ax, sg in ((0, 1.0), (0, -1.0), (2, 1.0), (2, -1.0)):
                p = np.array([cx, ycap, cz], F32); p[ax] += F32(sg) * r
                n = np.zeros(3, F32); n[ax], n[1] = sg, sy
                if c.Capped:                                        # through the rim: cap against side
                    parts.append(place(p, n, [ax, 1], "cyl_rim"))
                g = np.zeros(3, F32); g[ax], g[1] = sg, -sy         # over the cap and past the side, touching the rim only
                parts.append(place(p, -g, [ax, 1], "cyl_rim_graze"))
        # tangent to the side, disc == 0: |o.x - cx| == r with the direction along z puts the origin in a plane of the cylinder's own box,
        # and no other tangent line has dyadic coordinates - a slab-NaN ray as well, lost wherever a node ends in that plane
        for ax, sg in ((0, 1.0), (0, -1.0)):
            o = np.array([cx + F32(sg) * r, F32(0.5) * (F32(c.YMin) + F32(c.YMax)), cz + F32(1.0)], F32)
            parts.append((pack(o, (0, 0, -4)), "slab:cyl_tangent", 0))
    for _, sp in of_type(s, Sphere):                               # tangent to a sphere: both roots equal
        c, r = np.array(sp.Center, F32), F32(sp.Radius)
        for ax, sg in ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0)):   # (the origin is in a plane of the sphere's own box: a slab-NaN ray as well)
            o = c.copy(); o[ax] += F32(sg) * r; o[2] += F32(1.0)
            parts.append((pack(o, (0, -0.0, -1)), "slab:sphere_tangent", ax))
        # 3 : 4 : 5 - a tangent ray off the box's planes, one unit before the tangent point: c = |q|^2 + 1 - r^2 = 1 still sees one ulp of o
        # A step of o[a] moves c by 2 |o[a] - c[a]| ulp(o[a]): seen when that is a whole ulp of |q|^2 + 1, `blunt:` otherwise.
        q = r * F32(0.2)
        for sx, sy in itertools.product((-1.0, 1.0), repeat=2):
            o = (c + np.array([3.0 * q * sx, 4.0 * q * sy, 1.0], F32)).astype(F32)
            seen = [2.0 * abs(float(o[a] - c[a])) * float(np.spacing(np.nextafter(np.abs(o[a]), F32(0)))) for a in (0, 1)]
            a = int(np.argmax(seen))
            parts.append((pack(o, (0, 0, -1)), ("exact:" if seen[a] >= float(np.spacing(F32(r * r + 1.0))) else "blunt:") + "sphere_tangent", a))
    for _, dk in of_type(s, Disk):                                 # the rim of a level disk: rr == r * r
        n = np.array(dk.Normal, F32)
        if n[1] != 0 and n[0] == 0 and n[2] == 0:
            c, r = np.array(dk.Center, F32), F32(dk.Radius)
            for ax, sg in ((0, 1.0), (0, -1.0), (2, 1.0), (2, -1.0)):
                o = c.copy(); o[ax] += F32(sg) * r; o[1] += F32(1.0)
                parts.append((pack(o, (0, -2, 0)), "exact:disk_rim", ax))
            if r == F32(1.25):
                for sx, sz in itertools.product((-1.0, 1.0), repeat=2):
                    parts.append((pack(c + np.array([0.75 * sx, 1.0, 1.0 * sz], F32), (-0.0, -1, 0)), "exact:disk_rim", 0))
    tris = of_type(s, Triangle)
    if tris:                                                        # the analytic triangles in the plane z = -16
        for x, y in ((9.0, 1.0), (9.5, 0.5), (8.5, 1.5)):
            parts.append((pack((x, y, -11), (0, 0, -1)), "exact:tri_edge", 0))
        parts.append((pack((13, 1, -11), (0, 0, -2)), "exact:tri_vertex", 0))
        for x, y, perp in ((12.5, 0.5, 0), (13.5, 0.5, 0), (13.5, 1.5, 0), (12.5, 1.5, 0), (8.0, 1.0, 0), (9.0, 0.0, 1)):
            parts.append((pack((x, y, -11), (-0.0, 0, -1)), "exact:tri_edge", perp))
    for _, m in of_type(s, Mesh):
        for (x, y, _), perp, label in _mesh_seams(np.asarray(m.Triangles, F32)):
            parts.append((pack((x, y, -20), (0, 0, -1)), "exact:" + label, perp))
    if not parts:
        return np.zeros((0, 8), F32), np.zeros(0, "U32"), np.zeros(0, np.int64)
    rays, labels, perp = _cat(parts)
    above = rays[:, 1] > 0                                          # (a ray from below the floor meets the floor first)
    return rays[above], labels[above], perp[above]


def _seam_points(name):
    """(point, perpendicular axis, label) of seam points a fan is aimed at"""
    s = scene(name)
    out = []
    for _, o in solid_boxes(s):
        for p, ns in _box_edges(o.Min, o.Max):
            out.append((p, int(np.nonzero(ns[0])[0][0]), "fan:box_edge" if len(ns) == 2 else "fan:box_corner"))
    for _, c in of_type(s, CylinderY):
        cx, cz, r = F32(c.Center[0]), F32(c.Center[2]), F32(c.Radius)
        for ycap in (F32(c.YMax), F32(c.YMin)):
            for ax, sg in ((0, 1.0), (0, -1.0), (2, 1.0), (2, -1.0)):
                p = np.array([cx, ycap, cz], F32); p[ax] += F32(sg) * r
                out.append((p, 1, "fan:cyl_rim"))
    for _, sp in of_type(s, Sphere):                               # the silhouette seen along -z: a fan straddles hit and miss
        c, r = np.array(sp.Center, F32), F32(sp.Radius)
        for ax, sg in ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0)):
            p = c.copy(); p[ax] += F32(sg) * r
            out.append((p, ax, "fan:sphere_limb"))
    for _, dk in of_type(s, Disk):
        c, r = np.array(dk.Center, F32), F32(dk.Radius)
        n = np.array(dk.Normal, F32)
        if n[0] != 0 and n[2] != 0:                                 # the tilted disk: rr == r * r where 2 u * u == 1 on its plane
            u = F32(np.sqrt(0.5))
            for sg in (1.0, -1.0):
                out.append((np.array([c[0] + F32(sg) * u, c[1], c[2] - F32(sg) * u], F32), 0, "fan:disk_tilted_rim"))
        elif n[1] != 0:
            for ax, sg in ((0, 1.0), (0, -1.0), (2, 1.0), (2, -1.0)):
                p = c.copy(); p[ax] += F32(sg) * r
                out.append((p, ax, "fan:disk_rim"))
    if of_type(s, Triangle):
        for x, y, perp in ((9.0, 1.0, 0), (9.5, 0.5, 0), (13.0, 1.0, 0), (12.5, 0.5, 0), (13.5, 1.5, 1), (8.0, 1.0, 0), (9.0, 0.0, 1)):
            out.append((np.array([x, y, -16.0], F32), perp, "fan:tri_edge"))
    for _, m in of_type(s, Mesh):
        for p, perp, label in _mesh_seams(np.asarray(m.Triangles, F32))[::3]:
            out.append((np.array(p, F32), perp, "fan:" + label))
    return out


def edge_tie_fans(name):
    """(rays, labels, fan): FAN rays per fan - d = target - o from an origin off the lattice, the origin moved -2 .. +2 ulps along the seam's
    perpendicular axis.  The origin's coordinate on that axis is larger in magnitude than the target's, so one ulp of it is at least the
    rounding of the hit point: the fan's five parallel rays step across the seam."""
    pts = _seam_points(name)
    rng = np.random.default_rng(7)
    rays, labels, fan = [], [], []
    for k, (p, perp, label) in enumerate(pts):
        for rep in range(2):
            off = rng.uniform(1.5, 6.0, 3) * rng.choice([-1.0, 1.0], 3)
            off[2] = abs(off[2]) + 2.0                             # from the +z side, where nothing stands in the way
            if p[1] + off[1] < 0.25: off[1] = -off[1]              # (above the floor)
            off[perp] = np.sign(p[perp] if p[perp] != 0 else 1.0) * (abs(off[perp]) + 4.0)          # |o| > |target| on the perpendicular axis
            o = (p + off.astype(F32)).astype(F32)
            d = (p - o).astype(F32)
            base = pack(o, d)
            for u in range(-2, 3):
                rays.append(nudged(base, perp, u)); labels.append(label); fan.append(2 * k + rep)
    if not rays:
        return np.zeros((0, 8), F32), np.zeros(0, "U32"), np.zeros(0, np.int64)
    return np.concatenate(rays).astype(F32), np.array(labels, dtype="U32"), np.array(fan)


def edge_tie(name):
    ex, le, _ = edge_tie_exact(name)
    fr, lf, fan = edge_tie_fans(name)
    room = max(0, MAX_RAYS - ex.shape[0]) // FAN * FAN
    return np.concatenate([ex[:MAX_RAYS], fr[:room]]).astype(F32), np.concatenate([le[:MAX_RAYS], lf[:room]])


# --------------------------------------------------------------------------------------------------------------------------- interval_end
PER_KIND = 36


def interval_base(name):
    """rays aimed at every object from drawn origins (tMin 0, tMax FLT_MAX): interval_end takes t from the oracle's answer to them"""
    s = scene(name)
    rng = np.random.default_rng(17)
    aims = []
    for i, o in enumerate(s.Objects):
        if isinstance(o, Sphere): a = [np.array(o.Center, F32)]
        elif isinstance(o, Plane): a = [np.array([20.0, 0.0, 6.0], F32), np.array([-20.0, 0.0, 3.0], F32)]
        elif isinstance(o, Disk): a = [np.array(o.Center, F32)]
        elif isinstance(o, XYRect): a = [np.array([(o.X0 + o.X1) / 2, (o.Y0 + o.Y1) / 2, o.Z], F32)]
        elif isinstance(o, XZRect): a = [np.array([(o.X0 + o.X1) / 2, o.Y, (o.Z0 + o.Z1) / 2], F32)]
        elif isinstance(o, YZRect): a = [np.array([o.X, (o.Y0 + o.Y1) / 2, (o.Z0 + o.Z1) / 2], F32)]
        elif isinstance(o, Box): a = [(np.array(o.Min, F32) + np.array(o.Max, F32)) / 2]
        elif isinstance(o, CylinderY):
            a = [np.array([o.Center[0], (o.YMin + o.YMax) / 2, o.Center[2]], F32), np.array([o.Center[0] + 0.25, o.YMax, o.Center[2]], F32)]
        elif isinstance(o, Triangle): a = [(np.array(o.A, F32) + np.array(o.B, F32) + np.array(o.C, F32)) / 3]
        elif isinstance(o, Mesh):
            t = np.asarray(o.Triangles, F32)
            a = list(t[rng.choice(t.shape[0], 12, replace=False)].mean(axis=1))
        elif isinstance(o, VolumeGrid):
            mn, mx, sz = grid_box(o)
            idx = np.argwhere(np.asarray(o.Cells)[..., 0] > 0)
            a = [mn + (c + 0.5).astype(F32) * sz for c in idx[rng.choice(idx.shape[0], min(12, idx.shape[0]), replace=False)]] if idx.size else []
        else: a = []
        aims += [(i, p) for p in a]
    rays = []
    for i, p in aims:
        for _ in range(12):
            off = rng.uniform(0.7, 5.0, 3) * rng.choice([-1.0, 1.0], 3)
            o = (p + off).astype(F32)
            if o[1] < 0.3: o[1] = F32(0.3) + abs(o[1])
            d = ((p + rng.uniform(-0.2, 0.2, 3)).astype(F32) - o).astype(F32)
            rays.append(np.concatenate([o, d]))
    return pack(np.array(rays, F32)[:, 0:3], np.array(rays, F32)[:, 3:6])


def interval_end(name, base, rec):
    """base = interval_base(name) and rec = the oracle's records of it.  For up to PER_KIND hits of every primitive kind the ray again with tMax in
    {prev(t), t, next(t)}, with tMin in the same three (one ulp, not a constant), with tMin == tMax == t, and with tMax = +inf against FLT_MAX.
    Labels: kind/which, the nine of one hit in a row."""
    s = scene(name)
    hit = np.nonzero(rec[:, 0] != 0)[0]
    kinds = np.array([kind_of(s, rec[i, 1], rec[i, 2]) for i in hit])
    rays, labels = [], []
    for kind in sorted(set(kinds)):
        sel = hit[kinds == kind]
        sel = sel[(rec[sel, 3] > 0) & (rec[sel, 3] < 1e30)][:PER_KIND]
        for i in sel:
            t = F32(rec[i, 3]); lo, hi = ulps(t, -1), ulps(t, 1)
            for which, tmin, tmax in (("tmax_prev", 0.0, lo), ("tmax_t", 0.0, t), ("tmax_next", 0.0, hi), ("tmin_prev", lo, FLT_MAX), ("tmin_t", t, FLT_MAX),
                                      ("tmin_next", hi, FLT_MAX), ("both_t", t, t), ("tmax_inf", 0.0, INF), ("tmax_fltmax", 0.0, FLT_MAX)):
                r = base[i].copy(); r[6], r[7] = tmin, tmax
                rays.append(r); labels.append(kind + "/" + which)
    if not rays:
        return np.zeros((0, 8), F32), np.zeros(0, "U32")
    return _cap(np.array(rays, F32), np.array(labels, dtype="U32"), 3, group=9)


# --------------------------------------------------------------------------------------------------------------------------- threshold
def _around(c, k=2):
    c = F32(c)
    return [ulps(c, j) for j in range(-k, k + 1)]


def _dot(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def _cross(a, b):
    return np.array([F32(a[1] * b[2]) - F32(a[2] * b[1]), F32(a[2] * b[0]) - F32(a[0] * b[2]), F32(a[0] * b[1]) - F32(a[1] * b[0])], F32)


def threshold_cases(name):
    """(rays, labels, q, cut): directions whose denominator or determinant lands on the binary32 neighbours of a routine's cut-off, on either side
    and on it.  q is the quantity the routine compares, evaluated here in binary32 from the NORMALISED direction in the routine's order of
    operations; cut the constant it is compared with.  An axis direction plus a component of the cut-off's size: 1 + e * e rounds to 1, so the
    normalisation leaves both components as they are."""
    s = scene(name)
    parts = []

    def emit(o, d, label, q, cut):
        parts.append((pack(o, d), label, F32(q), F32(cut)))

    for sign in (1.0, -1.0):
        for _, pl in of_type(s, Plane)[:1]:                         # |n . d| against 1e-6 (Surfaces.cs:39-71); the floor, n = +y
            for e in _around(1e-6):
                d = np.array([1.0, -sign * e, 0.0], F32)
                emit((-30.0, sign * 2.0 ** -12, 30.0), d, "plane", abs(_dot(normalized(pl.Normal)[0], normalized(d)[0])), 1e-6)
        for _, dk in of_type(s, Disk):                              # |n . d| against 1e-6 (Surfaces.cs:108-142)
            n = normalized(dk.Normal)[0]
            if n[1] == 0: continue
            for e in _around(1e-6):
                d = np.array([1.0, -sign * e, 0.0], F32)
                o = np.array(dk.Center, F32); o[1] = ulps(o[1], int(sign))
                emit(o, d, "disk", abs(_dot(n, normalized(d)[0])), 1e-6)
        for _, rc in of_type(s, (XYRect, XZRect, YZRect)):          # |d.k| against 1e-8 (Surfaces.cs:184-214, 256-286, 328-358)
            if isinstance(rc, XZRect): axis, k, c = 1, rc.Y, ((rc.X0 + rc.X1) / 2, rc.Y, (rc.Z0 + rc.Z1) / 2)
            elif isinstance(rc, XYRect): axis, k, c = 2, rc.Z, ((rc.X0 + rc.X1) / 2, (rc.Y0 + rc.Y1) / 2, rc.Z)
            else: axis, k, c = 0, rc.X, (rc.X, (rc.Y0 + rc.Y1) / 2, (rc.Z0 + rc.Z1) / 2)
            along = (axis + 1) % 3
            for e in _around(1e-8):
                d = np.zeros(3, F32); d[along], d[axis] = 1.0, -sign * e
                o = np.array(c, F32); o[axis] = ulps(o[axis], int(sign))
                emit(o, d, "rect", abs(normalized(d)[0][axis]), 1e-8)
        for _, cy in of_type(s, CylinderY):
            if cy.Capped:                                           # |d.y| against 1e-8, exclusive (BoundedObjects.cs:148-247)
                for e in _around(1e-8):
                    d = np.array([1.0, sign * e, 0.0], F32)
                    y = F32(cy.YMin) if sign > 0 else F32(cy.YMax)
                    emit((cy.Center[0] - 0.5, ulps(y, -int(sign)), cy.Center[2]), d, "cylinder_cap", abs(normalized(d)[0][1]), 1e-8)
            for e in _around(1e-6, 3):                              # d.x * d.x + d.z * d.z against 1e-12
                d = np.array([sign * e, 1.0, 0.0], F32)
                dn = normalized(d)[0]
                emit((cy.Center[0] + 0.5, -1.0, cy.Center[2]), d, "cylinder_side", F32(F32(dn[0] * dn[0]) + F32(dn[2] * dn[2])), 1e-12)
    tri = [(np.array(t.A, F32), np.array(t.B, F32), np.array(t.C, F32), "triangle") for _, t in of_type(s, Triangle)[:2]]
    for _, m in of_type(s, Mesh):
        t = np.asarray(m.Triangles, F32)
        if np.ptp(t[..., 2]) == 0:                                  # the level mesh: +x lies in its plane
            tri += [(t[k, 0], t[k, 1], t[k, 2], "mesh_triangle") for k in (0, 1)]
    for A, B, Cc, label in tri:                                    # |det| against 1e-8 (Triangle.cs:131-175; MeshBVH.cs:239-304)
        e1, e2 = (B - A).astype(F32), (Cc - A).astype(F32)
        coef = abs(_dot(e1, _cross(np.array([0, 0, 1], F32), e2)))  # det = coef * d.z for a direction (1, 0, d.z) in the plane z = const
        for sign in (1.0, -1.0):
            for e in _around(F32(1e-8) / coef, 3):
                d = np.array([1.0, 0.0, -sign * e], F32)
                o = (A + (e1 + e2) * F32(0.25)).astype(F32); o[2] = ulps(o[2], int(sign))
                emit(o, d, label, abs(_dot(e1, _cross(normalized(d)[0], e2))), 1e-8)
    for _, g in of_type(s, VolumeGrid)[:3]:                        # |d.k| against 1e-12: VolumeGrid.Slab's parallel test (VolumeGrid.cs:331-355)
        mn, mx, sz = grid_box(g)
        for sign in (1.0, -1.0):
            for e in _around(1e-12):
                for oy in (mn[1], mn[1] + sz[1] * F32(1.5), mx[1], mx[1] + F32(1.0)):
                    d = np.array([1.0, sign * e, 0.0], F32)
                    emit((mn[0] - 2.0, oy, mn[2] + sz[2] * F32(2.5)), d, "grid_slab", abs(normalized(d)[0][1]), 1e-12)
    return _cat(parts)


def threshold(name):
    r, l, _, _ = threshold_cases(name)
    return _cap(r, l, 4)


# --------------------------------------------------------------------------------------------------------------------------- voxel_seam
_AXES = [np.array(v, F32) for v in ((1, 0, 0), (-1, -0.0, 0), (0, 2, -0.0), (-0.0, -0.5, 0), (0, -0.0, 4), (-0.0, 0, -1))]
_DIAG = [np.array(v, F32) for v in itertools.product((-1, 0, 1), repeat=3) if np.count_nonzero(v) >= 2]


def voxel_seam(name):
    """origins exactly on cell faces, edges and corners - inside solid and air cells, on a grid's outer faces, on the face two chunks share -
    along axes and symmetric diagonals, so that t_max_x == t_max_y (== t_max_z) step after step; rays along a cell-face plane of a whole grid
    and in through a grid's edge (enter_axis ties); hit points at wire_width_frac * voxel from a cell edge and its binary64 neighbours; tMin
    beyond the entry and inside a solid cell, tMax at a cell boundary"""
    s = scene(name)
    grids = of_type(s, VolumeGrid)
    if not grids:
        return np.zeros((0, 8), F32), np.zeros(0, "U32")
    rng = np.random.default_rng(23)
    parts = []
    dirs = _AXES + _DIAG
    for gi, (_, g) in enumerate(grids):
        mn, mx, sz = grid_box(g)
        n = np.asarray(g.Cells).shape[:3]
        lat = []
        for k in range(260):                                        # lattice points: corners, edge and face midpoints of cells, the outer faces included
            c = np.array([rng.integers(0, n[a] + 1) for a in range(3)])
            half = rng.integers(0, 2, 3) * (rng.random() < 0.6)
            if half.all(): half[rng.integers(0, 3)] = 0
            if k % 4 == 0: c[rng.integers(0, 3)] = rng.choice([0, n[0]]) if n[0] == n[1] == n[2] else 0
            lat.append((mn + (c + 0.5 * half).astype(F32) * sz).astype(F32))
        for k, p in enumerate(lat):
            for d in (dirs[(3 * k) % len(dirs)], dirs[(3 * k + 1) % len(dirs)], dirs[(7 * k + 2) % len(dirs)], _DIAG[(11 * k) % len(_DIAG)]):
                parts.append((pack(p, d), "lattice"))
                parts.append((pack(p - F32(2.0) * np.sign(d).astype(F32) * sz * (d != 0), d), "lattice_from_outside" if k % 4 == 0 else "lattice"))
        for j in range(0, n[1] + 1, 2):                             # along a cell-face plane of the whole grid, and in through a grid edge
            for kz in (1, n[2] - 2):
                z = mn[2] + sz[2] * F32(kz + 0.5)
                parts.append((pack((mn[0] - F32(2.0), mn[1] + sz[1] * F32(j), z), (1, 0, -0.0)), "face_plane"))
                parts.append((pack((mx[0] + F32(2.0), mn[1] + sz[1] * F32(j), z), (-1, -0.0, 0)), "face_plane"))
                parts.append((pack((mn[0] - F32(2.0), mn[1] - F32(2.0), z), (1, 1, 0)), "grid_edge"))
                parts.append((pack((mx[0] + F32(2.0), mx[1] + F32(2.0), z), (-1, -1, -0.0)), "grid_edge"))
                parts.append((pack((mn[0] - F32(2.0), mx[1] + F32(2.0), mn[2] - F32(2.0)), (1, -1, 1)), "grid_edge"))
        for j in range(n[1]):                                       # the interval against the cell walk: along +x through row (j, 1)
            o = (mn[0] - F32(2.0), mn[1] + sz[1] * F32(j + 0.5), mn[2] + sz[2] * F32(1.5))
            for tmin, tmax in ((2.0 + 2.5 * sz[0], FLT_MAX), (2.0 + 3.0 * sz[0], FLT_MAX), (0.0, 2.0 + 4.0 * sz[0]), (2.0 + 1.0 * sz[0], 2.0 + 1.0 * sz[0]),
                               (2.0 + 5.0 * sz[0], 2.0 + 7.0 * sz[0]), (0.0, 2.0), (ulps(F32(2.0), -1), ulps(F32(2.0), -1))):
                parts.append((pack(o, (4, 0, 0), tmin, tmax), "interval"))
        if g.EnableWireframe:                                       # straight down on the top faces of one cell column: x at the width from the cell's edge
            lo_x = [mn[0] + sz[0] * F32(i) for i in range(n[0])]
            w = F32(F32(WIRE_FRAC) * sz[0])
            for i, lo in enumerate(lo_x):
                x0 = F32(lo + w)
                xs = [x0, ulps(x0, 1), ulps(x0, -1)]
                if x0 == 0:                                         # the cell whose edge is at -w: binary64's neighbours of w are reachable around x = 0
                    xs += [F32(2.0 ** -55), F32(-2.0 ** -56), F32(-0.0), F32(2.0 ** -60)]
                for x in xs:
                    for kz in range(n[2]):
                        parts.append((pack((x, mx[1] + F32(2.0), mn[2] + sz[2] * F32(kz + 0.5)), (0, -1, 0)), "wire"))
    rays, labels = _cat(parts)
    keep = np.ones(rays.shape[0], bool)
    if rays.shape[0] > MAX_RAYS:                                    # every wire, interval, plane and edge ray; a seeded choice of the lattice
        lat = np.nonzero(np.char.startswith(labels, "lattice"))[0]
        drop = np.random.default_rng(5).choice(lat, rays.shape[0] - MAX_RAYS, replace=False)
        keep[drop] = False
    return rays[keep], labels[keep]


def dda_trace(g, ray):
    """VolumeGrid.Hit's cell walk (VolumeGrid.cs:99-231) restated for what voxel_seam is about: (tied steps, set of last_axis values chosen at a
    tied step, hit?, hit cell, last_axis, hit point).  A step is tied when the smallest t_max is shared by two or three axes."""
    o = ray[0:3].astype(F32); d = normalized(ray[3:6])[0]; tmin, tmax = F32(ray[6]), F32(ray[7])
    cells = np.asarray(g.Cells)[..., 0]
    n = cells.shape
    mn, mx, sz = grid_box(g)
    t_enter, t_exit, enter_axis = F32(-np.inf), F32(np.inf), -1
    none = (0, set(), False, None, -1, None)
    with np.errstate(all="ignore"):
        for a in range(3):
            if abs(d[a]) < F32(1e-12):
                if o[a] < mn[a] or o[a] > mx[a]: return none
                continue
            inv = F32(F32(1.0) / d[a])
            t0, t1 = F32(F32(mn[a] - o[a]) * inv), F32(F32(mx[a] - o[a]) * inv)
            if t0 > t1: t0, t1 = t1, t0
            if t0 > t_enter: t_enter, enter_axis = t0, a
            if t1 < t_exit: t_exit = t1
            if not (t_exit >= t_enter): return none
        if not (t_exit >= max(F32(0), t_enter)): return none
        t = t_enter
        if t < tmin: t = tmin
        if t > tmax or t > t_exit: return none
        t = F32(t + F32(1e-6))
        p = [F32(o[a] + F32(d[a] * t)) for a in range(3)]
        idx = [min(max(int(np.floor(F32(F32(p[a] - mn[a]) / sz[a]))), 0), n[a] - 1) for a in range(3)]
        step = [1 if d[a] > 0 else -1 if d[a] < 0 else 0 for a in range(3)]
        inv_d = [F32(0) if step[a] == 0 else F32(F32(1.0) / d[a]) for a in range(3)]
        nxt = [F32(mn[a] + (F32(F32(idx[a] + 1) * sz[a]) if step[a] > 0 else F32(F32(idx[a]) * sz[a]))) for a in range(3)]
        t_max = [F32(np.inf) if step[a] == 0 else F32(F32(nxt[a] - o[a]) * inv_d[a]) for a in range(3)]
        t_delta = [F32(np.inf) if step[a] == 0 else F32(abs(F32(sz[a] * inv_d[a]))) for a in range(3)]
        pick = lambda: 0 if (t_max[0] <= t_max[1] and t_max[0] <= t_max[2]) else 1 if t_max[1] <= t_max[2] else 2
        last_axis = pick() if enter_axis < 0 else enter_axis
        ties, tie_axes = 0, set()
        while t <= t_exit and t <= tmax:
            if cells[idx[0], idx[1], idx[2]] > 0:
                ht = max(t, tmin)
                return ties, tie_axes, True, tuple(idx), last_axis, np.array([F32(o[a] + F32(d[a] * ht)) for a in range(3)], F32)
            a = pick()
            m = min(t_max)
            if np.isfinite(m) and sum(1 for v in t_max if v == m) >= 2:
                ties += 1; tie_axes.add(a)
            idx[a] += step[a]; t = t_max[a]; t_max[a] = F32(t_max[a] + t_delta[a]); last_axis = a
            if not all(0 <= idx[k] < n[k] for k in range(3)): break
    return ties, tie_axes, False, None, last_axis, None


def wire_distance(g, cell, axis, p):
    """VolumeGrid.IsWireOnFace's binary64 edge distances (VolumeGrid.cs:256-296) of a hit point on the face `axis` of `cell`:
    (smallest distance to an edge of the face, the width it is compared with)"""
    mn, _, sz = grid_box(g)
    ww = min(0.5, max(0.0, float(F32(g.WireWidthFraction))))
    others = [a for a in range(3) if a != axis]
    dist = []
    for a in others:
        lo = float(F32(mn[a] + F32(F32(cell[a]) * sz[a]))); hi = lo + float(sz[a])
        dist.append(min(max(float(p[a]) - lo, 0.0), max(hi - float(p[a]), 0.0)))
    return min(dist), float(F32(F32(ww) * min(sz[others[0]], sz[others[1]])))


# --------------------------------------------------------------------------------------------------------------------------- batches, frames
def class_rays(name, cls, oracle_renderer):
    """the rays of one class on one scene; the oracle's renderer serves the classes that start from its trees or from a first answer"""
    if cls == "slab_nan":
        return slab_nan(name, seam_boxes(name, oracle_renderer))
    if cls == "edge_tie":
        return edge_tie(name)
    if cls == "interval_end":
        base = interval_base(name)
        return interval_end(name, base, oracle_records(oracle_renderer, base)[1])
    if cls == "threshold":
        return threshold(name)
    if cls == "voxel_seam":
        return voxel_seam(name)
    raise KeyError(cls)


def interleaved(batches):
    """the rays of several classes dealt round-robin into one batch: a wavefront then holds rays of every class side by side"""
    batches = [b for b in batches if b.shape[0]]
    n = max(b.shape[0] for b in batches)
    rows = [b[k] for k in range(n) for b in batches if k < b.shape[0]]
    return np.array(rows, F32)


def tree_boxes(name, oracle_renderer):
    """(m, 6) boxes of every node of the oracle's scene tree and mesh trees: what BVH.BoxHitFast / MeshBVH.BoxHitFast are asked about"""
    from yetanotherconsolegameengine_amd import abi
    out = [np.concatenate([n["min"], n["max"]]) for n in oracle_renderer.accel(abi.ACCEL_SCENE_NODES)]
    for k in range(len(of_type(scene(name), Mesh))):
        out += [np.concatenate([n["min"], n["max"]]) for n in oracle_renderer.accel(abi.ACCEL_MESH_NODES, k)]
    return np.array(out, F32).reshape(-1, 6)


# camera positions exactly on seams, for whole frames (yaw 0 looks down -z): (scene, kind of seam, position, yaw, pitch)
FRAME_POSES = [
    ("analytic", "box_plane", (-7.0, 1.0, -6.0), 0.0, 0.0),
    ("analytic", "box_corner", (-8.0, 2.0, -6.0), 0.5, -0.25),
    ("analytic", "sphere_centre", (0.0, 2.0, -8.0), 0.0, 0.0),
    ("analytic", "floor_plane", (2.0, 0.0, 0.0), 0.0, 0.125),
    ("analytic", "shared_box_face", (-6.0, 1.0, -7.0), 0.0, 0.0),
    ("mixed", "mesh_vertex", (2.0, 2.0, -23.25), 0.5, 0.0),          # of the uneven mesh: column 3, row 3, three quarters forward
    ("mixed", "mesh_vertex", (6.0, 2.0, -24.0), -0.5, 0.125),        # of the level mesh
    ("mixed", "grid_corner", (-8.0, 8.0, -24.0), 0.0, -0.5),
    ("voxels", "cell_corner", (-4.125, 4.0, -4.0), 0.0, 0.0),
    ("voxels", "cell_corner", (-3.125, 5.0, -3.0), 1.0, -0.25),
    ("voxels", "shared_chunk_face", (-0.125, 4.0, 4.5), 0.0, -1.0),
    ("voxels", "grid_corner", (-8.125, 8.0, 8.0), -0.75, -0.5),
]
N_FRAME_POSES = len(FRAME_POSES) + 3


def frame_poses(oracle_renderer_of):
    """FRAME_POSES and the three positions that are read off the scenes: on a plane of an inner node of `analytic`'s scene tree
    (oracle_renderer_of(name) -> an oracle renderer of the scene), on the corner of a solid voxel and of an air voxel"""
    from yetanotherconsolegameengine_amd import abi
    poses = list(FRAME_POSES)
    nodes = oracle_renderer_of("analytic").accel(abi.ACCEL_SCENE_NODES)
    nd = [n for n in nodes[1:] if n["count"] == 0 and np.abs(n["max"]).max() < 100][0]
    poses.append(("analytic", "node_plane", (float(nd["max"][0]), 1.5, float(nd["max"][2]) + 6.0), 0.0, 0.0))
    g = of_type(scene("voxels"), VolumeGrid)[0][1]
    mn, _, sz = grid_box(g)
    cells = np.asarray(g.Cells)[1:7, 1:7, 1:7, 0]
    for kind, want in (("solid_cell_corner", True), ("air_cell_corner", False)):
        c = np.argwhere((cells > 0) == want)[3] + 1
        poses.append(("voxels", kind, tuple(float(v) for v in (mn + c.astype(F32) * sz)), 0.25, -0.125))
    assert len(poses) == N_FRAME_POSES
    return poses
