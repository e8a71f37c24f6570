"""MeshScenes.AddMeshAutoGround behind its parse (Scenes/MeshScenes.cs:173-184, 233-330), restated in Python on parsed arrays: the yardstick
of ycge_obj_ground_host, ycge_obj_ground and ycge_obj_triangles_auto_ground.  It shares nothing with mesh_loader.py or the library: the
reference's own union-find with rank, a dict in insertion order, a float32 running sum (np.cumsum over float32 adds in order, one rounded
add per term), and the bounds over the kept faces' vertices.

One convention is not the reference's: the sign of a zero extreme.  The reference's follows HashSet enumeration order; here -0 orders
below +0, as include/ycge.h states (it cannot reach AddMeshAutoGround: t - (+-0 * scale) + 0.01f is the same value for either sign).
"""
import numpy as np

f32 = np.float32


def _components(n_positions, faces):
    """MeshScenes.cs:238-258 -> {root: [face indices]} in insertion order"""
    parent = list(range(n_positions))
    rank = [0] * n_positions

    def find(x):
        while x != parent[x]:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(x, y):
        rx, ry = find(x), find(y)
        if rx == ry:
            return
        if rank[rx] < rank[ry]:
            parent[rx] = ry
        elif rank[rx] > rank[ry]:
            parent[ry] = rx
        else:
            parent[ry] = rx
            rank[rx] += 1

    for a, b, c in faces:
        union(a, b)
        union(b, c)
    comp = {}
    for i, (a, b, c) in enumerate(faces):
        r = find(a)
        lst = comp.get(r)
        if lst is None:
            lst = comp[r] = []
        lst.append(i)
    return comp


def _ordered(x):
    """float32 array -> uint32 keys of the same order, -0 below +0"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _extremes(x):
    """min, max of a float32 vector: they start at +inf / -inf, NaN never replaces one, -0 orders below +0"""
    x = x[~np.isnan(x)]
    if x.size == 0:
        return f32(np.inf), f32(-np.inf)
    k = _ordered(x)
    return x[int(np.argmin(k))], x[int(np.argmax(k))]


def ground(pos, faces) -> dict:
    """-> min[3], max[3], centroid[3] (float32 arrays), extent (float32), n_components, component_faces, component_vertices, first_face"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    assert len(pos) > 0 and len(faces) > 0 and faces.min() >= 0 and faces.max() < len(pos)
    comp = _components(len(pos), faces.tolist())
    best_root, best_count = -1, -1
    for root, lst in comp.items():          # (.NET's Dictionary enumerates in insertion order; a strict >)
        if len(lst) > best_count:
            best_count, best_root = len(lst), root
    kept = faces[np.asarray(comp[best_root], np.int64)]
    with np.errstate(all="ignore"):
        third = f32(1.0) / f32(3.0)
        a, b, c = pos[kept[:, 0]], pos[kept[:, 1]], pos[kept[:, 2]]
        terms = ((a + b) + c) * third                                             # each operation rounded to binary32
        run = np.cumsum(np.vstack([np.zeros((1, 3), np.float32), terms]), axis=0, dtype=np.float32)   # cx = 0.0f; cx += term, in file order
        centroid = (run[-1] * (f32(1.0) / f32(len(kept)))).astype(np.float32)
        used = np.unique(kept.reshape(-1))
        rel = (pos[used] - centroid).astype(np.float32)
        ext = [_extremes(rel[:, k]) for k in range(3)]
        rmin = np.array([e[0] for e in ext], np.float32)
        rmax = np.array([e[1] for e in ext], np.float32)
        r = (rmax - rmin).astype(np.float32)
        extent = r[0]
        if r[1] > extent:
            extent = r[1]
        if r[2] > extent:
            extent = r[2]
        if extent <= f32(0.0):
            extent = f32(1.0)
        s = f32(1.0) / extent
        mn, mx = (rmin * s).astype(np.float32), (rmax * s).astype(np.float32)
    return dict(min=mn, max=mx, centroid=centroid, extent=f32(extent), n_components=len(comp), component_faces=int(best_count),
                component_vertices=int(len(used)), first_face=int(comp[best_root][0]))


def y_translate(min_y, scale, target_y):
    """AddMeshAutoGround (MeshScenes.cs:181): targetPos.Y - minYNormalized * scale + 0.01f, each operation rounded to binary32"""
    with np.errstate(all="ignore"):
        return (f32(target_y) - f32(min_y) * f32(scale)) + f32(0.01)


def words(info) -> list:
    """a ycge_obj_ground_info as comparable words: the ten floats as uint32, then the integer fields but on_device"""
    f = np.array(list(info.min) + list(info.max) + list(info.centroid) + [info.extent], np.float32).view(np.uint32).tolist()
    return f + [info.n_components, info.component_faces, info.component_vertices, info.first_face]


def want_words(w) -> list:
    """ground()'s answer as the same words"""
    f = np.concatenate([w["min"], w["max"], w["centroid"], [w["extent"]]]).astype(np.float32).view(np.uint32).tolist()
    return f + [w["n_components"], w["component_faces"], w["component_vertices"], w["first_face"]]
