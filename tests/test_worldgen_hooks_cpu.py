"""Not gpu: the pieces of csrc/ycge_worldgen.h that no chunk can tell apart from a wrong version, on inputs of the test's own, through
the host hooks of include/ycge_hooks.h - against tests/worldgen_restatement.py.  The river step above all: with the reference's threshold
of 50 against an accumulation of at most 9 it never alters a cell, so only these tests hold wg::d8_direction, wg::river_accum (the
in-degree restatement, against the LITERAL ascending sort) and wg::river_carve (the carve and river-surface formulas)."""
import ctypes as C

import numpy as np
import pytest

import worldgen_restatement as R
from yetanotherconsolegameengine_amd import abi

I32P, F32P, U32P = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def _p(a, t):
    return a.ctypes.data_as(t)


@pytest.fixture(scope="module")
def hooks(product_lib):
    L = product_lib
    L.ycge_host_worldgen_noise.restype, L.ycge_host_worldgen_noise.argtypes = C.c_int, [C.c_int32, I32P, I32P, F32P, F32P, C.c_int32, U32P, F32P]
    L.ycge_host_worldgen_height.restype, L.ycge_host_worldgen_height.argtypes = C.c_int, [C.c_void_p, C.c_int32, I32P, I32P, I32P]
    L.ycge_host_worldgen_river.restype, L.ycge_host_worldgen_river.argtypes = C.c_int, [I32P, C.c_int32, C.c_int32, I32P, F32P, I32P, I32P]
    L.ycge_host_worldgen_carve.restype, L.ycge_host_worldgen_carve.argtypes = C.c_int, [C.c_float, C.c_int32, C.c_int32, I32P, I32P]
    return L


def _river(L, tile, size, sea):
    t = np.ascontiguousarray(tile, np.int32)
    d, a = np.zeros((size, size), np.int32), np.zeros((size, size), np.float32)
    c, w = np.zeros((size, size), np.int32), np.zeros((size, size), np.int32)
    assert L.ycge_host_worldgen_river(_p(t, I32P), size, sea, _p(d, I32P), _p(a, F32P), _p(c, I32P), _p(w, I32P)) == 0
    return d, a, c, w


@pytest.mark.parametrize("size,levels,seed", [(8, 2, 1), (12, 3, 2), (16, 4, 3), (9, 1, 4), (32, 6, 5), (5, 40, 6)])
def test_river_step_of_the_library_equals_the_literal_sort_on_tiles_with_many_ties(hooks, size, levels, seed):
    rng = np.random.default_rng(seed)
    tile = rng.integers(0, levels, (size + 2, size + 2)).astype(np.int64)
    dnx, dnz = R.d8(tile, size)
    literal = R.river_accum_sorted(tile[1:-1, 1:-1], dnx, dnz)
    d, a, c, w = _river(hooks, tile, size, 7)
    assert np.array_equal(d, (dnx + 1) * 3 + (dnz + 1))          # D8: oz outer, ox inner, the first of equal drops
    assert np.array_equal(a, literal) and a.max() <= 9            # in-degree (+ 1 for a pit) == the ascending sort and push
    assert np.array_equal(a, R.river_accum_indegree(dnx, dnz))
    # ... whatever order the sort leaves equal heights in (Array.Sort is not stable): ties reversed
    order = sorted(((int(tile[1 + x, 1 + z]), -x, -z) for x in range(size) for z in range(size)))
    acc = np.zeros((size, size), np.float32)
    for _, mx, mz in order:
        x, z = -mx, -mz
        v = acc[x, z] if acc[x, z] > 0 else np.float32(1)
        nx, nz = x + int(dnx[x, z]), z + int(dnz[x, z])
        if 0 <= nx < size and 0 <= nz < size:
            acc[nx, nz] += v
    assert np.array_equal(acc, a)
    assert np.array_equal(c, tile[1:-1, 1:-1]) and (w == 7).all()          # below the threshold nothing is carved, the river surface is the sea


def test_a_pit_with_eight_neighbours_draining_into_it_counts_nine(hooks):
    tile = np.full((5, 5), 3, np.int64)
    tile[2, 2] = 0
    d, a, c, w = _river(hooks, tile, 3, 1)
    assert a[1, 1] == 9 and d[1, 1] == 4 and (a.sum() == 9)


def test_carve_and_river_surface_formulas_behind_the_threshold(hooks):
    for accum in (0.0, 9.0, 50.0, 50.5, 64.0, 64.5, 75.0, 78.6, 92.9, 100.0, 150.0, 1e6):
        for ground, sea in ((80, 64), (3, 64), (2, 1), (66, 64), (0, 5)):
            c, w = C.c_int32(), C.c_int32()
            assert hooks.ycge_host_worldgen_carve(accum, ground, sea, C.byref(c), C.byref(w)) == 0
            rc, rw = R.carve_and_surface(np.float32(accum), np.int64(ground), sea)
            assert (c.value, w.value) == (int(rc), int(rw)), (accum, ground, sea)
    c, w = C.c_int32(), C.c_int32()
    hooks.ycge_host_worldgen_carve(100.0, 80, 64, C.byref(c), C.byref(w))
    assert (c.value, w.value) == (77, 79)          # t = 1: carve 3.5 -> bed 80 - 3, surface bed + ceil(2.0)


def test_hash_and_gradient_noise_known_answers(hooks):
    rng = np.random.default_rng(11)
    ix = np.concatenate([rng.integers(-2 ** 31, 2 ** 31, 200), [0, -1, 1, 2 ** 31 - 1, -2 ** 31]]).astype(np.int32)
    iz = np.concatenate([rng.integers(-2 ** 31, 2 ** 31, 200), [0, -1, -7, 5, 3]]).astype(np.int32)
    x = np.concatenate([rng.uniform(-300, 300, 150), rng.uniform(-1, 1, 50), [0.0, 3.0, -2.0, -7.0, -0.25]]).astype(np.float32)
    z = np.concatenate([rng.uniform(-300, 300, 150), rng.uniform(-1, 1, 50), [0.0, -4.0, 5.0, -1.0, -1.75]]).astype(np.float32)
    for seed in (0, 11, -5, 2 ** 31 - 1):
        h, n = np.zeros(205, np.uint32), np.zeros(205, np.float32)
        assert hooks.ycge_host_worldgen_noise(205, _p(ix, I32P), _p(iz, I32P), _p(x, F32P), _p(z, F32P), seed, _p(h, U32P), _p(n, F32P)) == 0
        assert np.array_equal(h, R.fast_hash(ix, 0, iz, seed))
        assert np.array_equal(n.view(np.uint32), R.gradient_noise2(x, z, seed).view(np.uint32))          # bit for bit, negative coordinates included
        assert np.array_equal(n[200:204], np.zeros(4, np.float32))                                       # a gradient noise vanishes on its lattice
    # FNV-1a over (x, 0, z) written out: offset ^ seed, then xor and multiply three times
    k = 2166136261 ^ 7
    for v in (5, 0, 0xFFFFFFFD):
        k = ((k ^ v) * 16777619) & 0xFFFFFFFF
    h1 = np.zeros(1, np.uint32); n1 = np.zeros(1, np.float32)
    hooks.ycge_host_worldgen_noise(1, _p(np.array([5], np.int32), I32P), _p(np.array([-3], np.int32), I32P), _p(np.zeros(1, np.float32), F32P),
                                   _p(np.zeros(1, np.float32), F32P), 7, _p(h1, U32P), _p(n1, F32P))
    assert int(h1[0]) == k


@pytest.mark.parametrize("size,chunks_y,seed", [(32, 8, 0), (12, 8, 5)])
def test_height_y_along_lines(hooks, size, chunks_y, seed):
    cfg = R.Config(size, chunks_y, seed)
    w = abi.World(size, chunks_y, seed, abi.Vec3(0, 0, 0), abi.Vec3(1, 1, 1))
    for gx, gz in ((np.arange(400, 520), np.full(120, 101)), (np.arange(-9700, -9500, 2), np.arange(-3000, -2800, 2)), (np.arange(9900, 10100, 2), np.full(100, -7)),
                   (np.full(60, -40), np.arange(-30, 30))):
        gx, gz = gx.astype(np.int32), gz.astype(np.int32)
        out = np.zeros(len(gx), np.int32)
        assert hooks.ycge_host_worldgen_height(C.byref(w), len(gx), _p(gx, I32P), _p(gz, I32P), _p(out, I32P)) == 0
        assert np.array_equal(out, R.height_y(gx.astype(np.int64), gz.astype(np.int64), cfg))
