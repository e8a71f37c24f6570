"""The pool of resident meshes (csrc/ycge_mesh_pool.h, behind ycge_scene_attach_meshes / ycge_scene_detach_meshes) as far as a box without a GPU
sees it: its allocator of unit ranges and mesh indices, through the context-free hook ycge_debug_mesh_ranges, against a restatement in Python
on drawn sequences of takes and gives - and the exports, prototypes and knobs the feature adds."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from yetanotherconsolegameengine_amd import abi

ROOT = Path(__file__).resolve().parents[1]
TAKE, GIVE, INDEX_TAKE, INDEX_GIVE = abi.MESH_RANGE_TAKE, abi.MESH_RANGE_GIVE, abi.MESH_INDEX_TAKE, abi.MESH_INDEX_GIVE


class Restatement:
    """The allocator said again: free ranges as a sorted list of [first, units], first fit by address, neighbours joined, a free range that
    reaches the records' end moves the end back; the lowest free index, free indices at the table's end dropped."""

    def __init__(self, end=0, n_index=0):
        self.free, self.end, self.free_index, self.n_index = [], end, set(), n_index

    def take(self, units):
        if units == 0:
            return self.end
        for k, (first, have) in enumerate(self.free):
            if have >= units:
                self.free[k:k + 1] = [[first + units, have - units]] if have > units else []
                return first
        first = self.end
        self.end += units
        return first

    def give(self, first, units):
        if units == 0:
            return
        self.free = sorted(self.free + [[first, units]])
        joined = []
        for f, u in self.free:
            if joined and joined[-1][0] + joined[-1][1] == f:
                joined[-1][1] += u
            else:
                joined.append([f, u])
        if joined and joined[-1][0] + joined[-1][1] == self.end:
            self.end = joined.pop()[0]
        self.free = joined

    def take_index(self):
        if self.free_index:
            i = min(self.free_index)
            self.free_index.remove(i)
            return i
        self.n_index += 1
        return self.n_index - 1

    def give_index(self, i):
        self.free_index.add(i)
        while self.n_index and self.n_index - 1 in self.free_index:
            self.n_index -= 1
            self.free_index.remove(self.n_index)


def _drawn_ops(seed, n_ops=2000, end0=0, n_index0=0):
    """takes and gives of 1..5 000 units (and now and then of none) with their indices, drawn against the restatement so that every give
    names a live range: (ops [n, 3], the restatement's answer per op [n, 4], what was live at the end)"""
    rng = np.random.default_rng(seed)
    R = Restatement(end0, n_index0)
    live = []          # (first, units, index)
    if end0:           # the records of an upload: n_index0 meshes one behind the other
        cuts = np.sort(rng.choice(np.arange(1, end0), n_index0 - 1, replace=False)) if n_index0 > 1 else np.array([], np.int64)
        edges = [0, *[int(c) for c in cuts], end0]
        live = [(edges[i], edges[i + 1] - edges[i], i) for i in range(n_index0)]
    ops, want = [], []

    def state(res):
        want.append((res, R.end, len(R.free), sum(u for _, u in R.free)))

    while len(ops) < n_ops:
        if live and (rng.random() < 0.45 or len(live) > 60):
            first, units, index = live.pop(int(rng.integers(len(live))))
            ops.append((GIVE, first, units)); R.give(first, units); state(0)
            ops.append((INDEX_GIVE, index, 0)); R.give_index(index); state(0)
        else:
            units = 0 if rng.random() < 0.03 else int(rng.integers(1, 5001))
            ops.append((INDEX_TAKE, 0, 0)); index = R.take_index(); state(index)
            ops.append((TAKE, units, 0)); first = R.take(units); state(first)
            live.append((first, units, index))
            # the restatement's own promises, checked where they are made
            assert index == min(set(range(R.n_index + 1)) - {i for _, _, i in live[:-1]}), "the lowest free index"
            spans = sorted((f, f + u) for f, u, _ in live if u)
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "two live ranges overlap"
    return np.asarray(ops, np.int64), np.asarray(want, np.int64), live


@pytest.mark.parametrize("seed,end0,n_index0", [(1, 0, 0), (2, 0, 0), (3, 70000, 9), (4, 1, 1)])
def test_the_allocator_equals_its_restatement_on_drawn_sequences(product_lib, seed, end0, n_index0):
    ops, want, live = _drawn_ops(seed, end0=end0, n_index0=n_index0)
    assert len(ops) >= 2000 and (ops[:, 0] == GIVE).sum() > 300 and (ops[:, 0] == TAKE).sum() > 300
    got = abi.mesh_ranges(ops, end0, n_index0, product_lib)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"op {bad[0]} {ops[bad[0]]}: the library says {got[bad[0]]}, the restatement {want[bad[0]]}"
    assert want[:, 2].max() >= 5, "the sequence never held several free ranges"
    # ranges were reused (a take answered below the end it started from) and the end moved back (a give that lowered it)
    takes = np.nonzero((ops[:, 0] == TAKE) & (ops[:, 1] > 0))[0]
    assert sum(got[k, 0] < got[k - 1, 1] for k in takes if k > 0) > 50
    gives = np.nonzero(ops[:, 0] == GIVE)[0]
    assert sum(got[k, 1] < got[k - 1, 1] for k in gives if k > 0) >= 3          # (with some forty live ranges a give seldom names the last one)


def test_neighbours_coalesce_and_the_first_fit_is_by_address(product_lib):
    run = lambda ops, end0=0, n0=0: abi.mesh_ranges(ops, end0, n0, product_lib)
    # five ranges of 10; the 2nd and the 4th go, then the 3rd between them: one free range of 30
    got = run([(TAKE, 10, 0)] * 5 + [(GIVE, 10, 10), (GIVE, 30, 10), (GIVE, 20, 10)])
    assert [int(v) for v in got[:5, 0]] == [0, 10, 20, 30, 40]
    assert [tuple(int(v) for v in r[1:]) for r in got[5:]] == [(50, 1, 10), (50, 2, 20), (50, 1, 30)]
    # first fit by address: free ranges of 30 at 10 and of 50 at 60 - 20 units go to 10, 40 to 60, 31 to the end
    got = run([(TAKE, 10, 0), (TAKE, 30, 0), (TAKE, 20, 0), (TAKE, 50, 0), (TAKE, 5, 0), (GIVE, 60, 50), (GIVE, 10, 30), (TAKE, 40, 0), (TAKE, 20, 0), (TAKE, 31, 0), (TAKE, 10, 0)])
    assert [int(v) for v in got[7:, 0]] == [60, 10, 115, 30]
    # the last range goes: the end moves back, over the free range before it too
    got = run([(TAKE, 10, 0), (TAKE, 20, 0), (TAKE, 30, 0), (GIVE, 10, 20), (GIVE, 30, 30)])
    assert tuple(int(v) for v in got[-1][1:]) == (10, 0, 0)
    # a mesh without triangles takes nothing and gives nothing
    got = run([(TAKE, 7, 0), (TAKE, 0, 0), (GIVE, 7, 0)])
    assert [tuple(int(v) for v in r) for r in got] == [(0, 7, 0, 0), (7, 7, 0, 0), (0, 7, 0, 0)]
    # indices: the lowest free one; free indices at the table's end go with it
    got = run([(INDEX_TAKE, 0, 0)] * 4 + [(INDEX_GIVE, 1, 0), (INDEX_GIVE, 2, 0), (INDEX_TAKE, 0, 0), (INDEX_GIVE, 3, 0), (INDEX_TAKE, 0, 0), (INDEX_TAKE, 0, 0)], 0, 2)
    assert [int(v) for v in got[:, 0]] == [2, 3, 4, 5, 0, 0, 1, 0, 2, 3]
    assert product_lib.ycge_debug_mesh_ranges(-1, 0, None, 0, None) == abi.YCGE_ERR_INVALID_ARG
    assert product_lib.ycge_debug_mesh_ranges(0, 0, None, 3, None) == abi.YCGE_ERR_INVALID_ARG


def test_exports_prototypes_and_documents(product_lib):
    names = ("ycge_scene_attach_meshes", "ycge_scene_detach_meshes", "ycge_scene_append_materials", "ycge_scene_attach_obj_mesh")
    header = (ROOT / "include" / "ycge.h").read_text()
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text()
    for n in names:
        assert n in abi.EXPORTED_SYMBOLS and hasattr(product_lib, n) and f"int {n}(ycge_ctx *ctx" in header, n
    for n in abi.MESH_POOL_HOOK_PROTOTYPES:
        assert hasattr(product_lib, n) and f"int {n}(" in hooks, n
    assert "#define YCGE_ABI_VERSION 10" in header
    # without a context the calls refuse and write nothing
    out = (C.c_int32 * 1)(-7)
    assert product_lib.ycge_scene_attach_meshes(None, None, 0, out) == abi.YCGE_ERR_INVALID_ARG and out[0] == -7
    assert product_lib.ycge_scene_detach_meshes(None, out, 1) == abi.YCGE_ERR_INVALID_ARG
    assert product_lib.ycge_scene_append_materials(None, None, 0, out) == abi.YCGE_ERR_INVALID_ARG and out[0] == -7
    assert product_lib.ycge_scene_attach_obj_mesh(None, 0, 1, 1.0, 1.0, None, 0, out, None) == abi.YCGE_ERR_INVALID_ARG and out[0] == -7
    # the sentence the feature retires
    integration = (ROOT / "INTEGRATION.md").read_text()
    assert "Only a new mesh or a new material still needs" not in integration
    assert "ycge_scene_attach_meshes" in integration and "ycge_scene_attach_meshes" in (ROOT / "README.md").read_text() and "ycge_mesh_pool" in (ROOT / "DESIGN.md").read_text()
