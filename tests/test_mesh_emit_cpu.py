"""The mesh arena assembled on the device (csrc/ycge_mesh_emit.hip, driven by csrc/ycge_mesh_bvh.cpp) as far as a box without a GPU sees it.

The kernels rest on ONE claim about the host's emit_mesh_records: the builder numbers a tree's nodes in pre-order, left before right, so the
depth-first emit lays the records out in node order - the 32-byte unit of node i is the exclusive prefix sum of the record sizes of the
nodes before it (2 units for an internal node's GNode, 3 * ((count + 1) / 2) for a leaf's triangle pair records).  That is restated here
in numpy and held against ycge_host_mesh_arena, bytes and all; it passes with or without the feature - it is the specification.  The
hooks of the feature are declared, exported and mirrored, and refuse without a device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from yetanotherconsolegameengine_amd import abi

ROOT = Path(__file__).resolve().parents[1]
HOOKS = ("ycge_debug_device_mesh_arena", "ycge_debug_read_mesh_arena", "ycge_debug_read_meshes", "ycge_debug_mesh_emit_stats")
f32 = np.float32
REF_MESH_NODE, REF_MESH_LEAF = 2, 3
NODE = np.dtype([("mn", "<f4", 3), ("mx", "<f4", 3), ("left", "<i4"), ("right", "<i4"), ("start", "<i4"), ("count", "<i4")])


def _host_tree(L, t9):
    n = len(t9)
    L.ycge_host_build_mesh.restype = C.c_int
    L.ycge_host_build_mesh.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    nodes = np.zeros(2 * n, NODE); leaf = np.zeros(n, np.int32); st = np.zeros(3, np.int32)
    k = L.ycge_host_build_mesh(t9.ctypes.data, n, nodes.ctypes.data, leaf.ctypes.data, st.ctypes.data)
    assert k >= 1 and st[0] == 0
    return nodes[:k], leaf


def _host_arena(L, t9):
    L.ycge_host_mesh_arena.restype = C.c_int
    L.ycge_host_mesh_arena.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    root = np.zeros(1, np.uint32)
    nbytes = L.ycge_host_mesh_arena(t9.ctypes.data, len(t9), None, 0, root.ctypes.data)
    assert nbytes > 0 and nbytes % 32 == 0
    arena = np.zeros(nbytes, np.uint8)
    assert L.ycge_host_mesh_arena(t9.ctypes.data, len(t9), arena.ctypes.data, nbytes, root.ctypes.data) == nbytes
    return arena, int(root[0])


def layout(nodes):
    """(unit, reference) per pre-order node, total units: the rule the kernels implement"""
    count = nodes["count"].astype(np.int64)
    size = np.where(count > 0, 3 * ((count + 1) // 2), 2)
    unit = np.cumsum(size) - size
    ref = np.where(count > 0, (REF_MESH_LEAF << 29) | (unit << 4) | count, (REF_MESH_NODE << 29) | (unit << 4)).astype(np.uint32)
    return unit, ref, int(size.sum())


def records(nodes, leaf, t9, material=0):
    """the arena of one mesh from the layout rule alone: no recursion, every record a function of its own node"""
    unit, ref, total = layout(nodes)
    words = np.zeros((total, 8), np.uint32)
    fl = words.view(f32)
    for i, nd in enumerate(nodes):
        u = int(unit[i])
        if nd["count"] <= 0:
            L, R = nodes[nd["left"]], nodes[nd["right"]]
            fl[u] = [L["mn"][0], L["mn"][1], L["mn"][2], L["mx"][2], L["mx"][0], L["mx"][1], R["mn"][0], R["mn"][1]]
            fl[u + 1, :4] = [R["mn"][2], R["mx"][2], R["mx"][0], R["mx"][1]]
            words[u + 1, 4:6] = [ref[nd["left"]], ref[nd["right"]]]
            continue
        for k in range(int(nd["count"])):
            ti = int(leaf[nd["start"] + k])
            v = t9[ti]
            rec = words[u + 3 * (k // 2): u + 3 * (k // 2) + 3].reshape(-1)          # 24 words: 9 component pairs, orig, material, padding
            vals = [v[0], v[1], v[2], v[3] - v[0], v[4] - v[1], v[5] - v[2], v[6] - v[0], v[7] - v[1], v[8] - v[2]]
            rec.view(f32)[np.arange(9) * 2 + (k & 1)] = np.asarray(vals, f32)
            rec[18 + (k & 1)] = ti
            rec[20 + (k & 1)] = material
    return words.reshape(-1).view(np.uint8), int(ref[0])


SIZES = (1, 2, 7, 8, 9, 17, 100, 333, 1000, 2048, 3001, 5000)


@pytest.mark.parametrize("n", SIZES)
def test_a_nodes_unit_is_the_exclusive_scan_of_the_record_sizes(product_lib, n):
    rng = np.random.default_rng(1000 + n)
    c = rng.uniform(-10, 10, (n, 1, 3)) * rng.choice([0.1, 1.0, 5.0])
    t9 = np.ascontiguousarray((c + rng.uniform(-0.3, 0.3, (n, 3, 3))).astype(f32).reshape(n, 9))
    nodes, leaf = _host_tree(product_lib, t9)
    # pre-order, left before right: a node's left child is the next node, its right child follows the whole left subtree
    inner = np.flatnonzero(nodes["count"] <= 0)
    assert (nodes["left"][inner] == inner + 1).all() and (nodes["right"][inner] > nodes["left"][inner]).all()
    arena, root = _host_arena(product_lib, t9)
    mine, my_root = records(nodes, leaf, t9)
    assert my_root == root
    assert len(mine) == len(arena), f"{n} triangles: {len(mine)} bytes by the scan, {len(arena)} on the host"
    assert np.array_equal(mine, arena), f"{n} triangles: first difference at byte {int(np.flatnonzero(mine != arena)[0])}"


def test_the_hooks_are_declared_exported_and_mirrored(product_lib):
    text = (ROOT / "include" / "ycge_hooks.h").read_text()
    for name in HOOKS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert getattr(product_lib, name) is not None
        assert name in abi.MESH_EMIT_HOOK_PROTOTYPES and name not in abi.EXPORTED_SYMBOLS
    assert len(abi.MESH_EMIT_STATS) == 4 and abi.MESH_EMIT_RES_WORDS == 8


def test_the_arena_hook_refuses_without_a_device(product_lib):
    """Without a GPU the hook refuses and writes nothing (with one it is held to the host's bytes: tests/test_gpu_mesh_emit_device.py)."""
    fn = product_lib.ycge_debug_device_mesh_arena
    fn.restype, fn.argtypes = abi.MESH_EMIT_HOOK_PROTOTYPES["ycge_debug_device_mesh_arena"]
    t9 = np.random.default_rng(1).uniform(-1, 1, (100, 9)).astype(f32)
    out = np.full(1 << 16, 0x5a, np.uint8); root = np.full(1, 0xdeadbeef, np.uint32); tl = np.full(1, 0xdeadbeef, np.uint32); res = np.full(8, 0xdeadbeef, np.uint32)
    rc = fn(t9.ctypes.data, 100, out.ctypes.data, out.nbytes, root.ctypes.data, tl.ctypes.data, res.ctypes.data)
    if product_lib.ycge_device_count() > 0:
        assert rc > 0 and res[1] >= 1
    else:
        assert rc in (abi.YCGE_ERR_NO_DEVICE_CODE, abi.YCGE_ERR_DEVICE), rc
        assert (out == 0x5a).all() and root[0] == 0xdeadbeef and tl[0] == 0xdeadbeef and (res == 0xdeadbeef).all()
    assert fn(t9.ctypes.data, 100, out.ctypes.data, out.nbytes, None, tl.ctypes.data, res.ctypes.data) in (abi.YCGE_ERR_INVALID_ARG, abi.YCGE_ERR_NO_DEVICE_CODE, abi.YCGE_ERR_DEVICE)


def test_the_knobs_parse_as_documented(product_lib, monkeypatch):
    fn = product_lib.ycge_debug_mesh_emit_stats
    fn.restype, fn.argtypes = abi.MESH_EMIT_HOOK_PROTOTYPES["ycge_debug_mesh_emit_stats"]

    def knobs():
        out = (C.c_int64 * 4)(-1, -1, -1, -1)
        assert fn(None, out) == abi.YCGE_ERR_INVALID_ARG
        return int(out[0]), int(out[1])
    for name in ("YCGE_MESH_EMIT_HOST", "YCGE_MESH_EMIT_DEVICE_MIN"):
        monkeypatch.delenv(name, raising=False)
    assert knobs() == (0, 16000)          # the default crossover is a measured number (profiles/mesh_build_rate.json)
    monkeypatch.setenv("YCGE_MESH_EMIT_HOST", "1")
    monkeypatch.setenv("YCGE_MESH_EMIT_DEVICE_MIN", "777")
    assert knobs() == (1, 777)
    assert fn(None, None) == abi.YCGE_ERR_INVALID_ARG
