"""ycge_obj_ground_host - the library's host tail of MeshScenes.AddMeshAutoGround, the yardstick and fallback of the kernels of
csrc/ycge_obj_ground.hip - against tests/obj_ground_restatement.py: uint32 views of the floats, every integer field, no tolerance.  No GPU
is touched: the device side is tests/test_gpu_obj_ground.py."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import obj_ground_cases as cases
import obj_ground_restatement as R
from obj_ground_cases import want_of
from obj_ground_restatement import want_words, words
from yetanotherconsolegameengine_amd import abi, mesh_loader

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "yetanotherconsolegameengine_amd" / "csrc"
NEW_EXPORTS = ("ycge_obj_ground_host", "ycge_obj_ground", "ycge_obj_triangles_auto_ground")
NEW_HOOKS = ("ycge_debug_obj_ground_stats", "ycge_debug_obj_ground_phases")


@pytest.fixture(scope="module")
def L():
    lib = abi.load_library()
    for name in NEW_EXPORTS:
        fn = getattr(lib, name)          # (AttributeError - a failure, not a skip - when the export is missing)
        fn.restype, fn.argtypes = abi._PROTOTYPES[name]
    return lib


@pytest.mark.parametrize("name", cases.NAMES)
def test_host_tail_equals_the_restatement(L, name):
    c = cases.get(name)
    pos, faces, info = abi.obj_parse_host(c.text, L)          # the text gives back the drawn arrays
    assert np.array_equal(pos.view(np.uint32), c.pos.view(np.uint32)) and np.array_equal(faces, c.faces), name
    got = abi.obj_ground_host(pos, faces, L)
    assert got.on_device == 0 and got.reserved == 0
    assert words(got) == want_words(want_of(name)), (name, words(got), want_words(want_of(name)))


@pytest.mark.parametrize("name", [n for n in cases.NAMES if n not in cases.ZERO_EXTREME + cases.NAN_CENTROID])
def test_restatement_equals_mesh_loader_where_no_extreme_is_a_zero(name):
    """(... and where the centroid is a number: mesh_loader takes its extremes with np.min / np.max, which hand a NaN on, while the
    reference's `x < rMin` is false for one - cases.NAN_CENTROID is held to the restatement and the host tail alone)"""
    c = cases.get(name)
    w = want_of(name)
    assert not (np.concatenate([w["min"], w["max"]]) == 0).any()
    with np.errstate(all="ignore"):
        mn, mx = mesh_loader.read_obj_bounds_normalized(c.pos, c.faces)
    assert np.array_equal(mn.view(np.uint32), w["min"].view(np.uint32)) and np.array_equal(mx.view(np.uint32), w["max"].view(np.uint32)), name


def test_argument_refusals(L):
    fn = L.ycge_obj_ground_host
    pos = np.zeros((3, 3), np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    info = abi.ObjGroundInfo()
    assert fn(pos.ctypes.data, 3, faces.ctypes.data, 1, C.byref(info)) == abi.YCGE_OK and info.component_faces == 1
    assert fn(None, 3, faces.ctypes.data, 1, C.byref(info)) == abi.YCGE_ERR_INVALID_ARG
    assert fn(pos.ctypes.data, 3, None, 1, C.byref(info)) == abi.YCGE_ERR_INVALID_ARG
    assert fn(pos.ctypes.data, 3, faces.ctypes.data, 1, None) == abi.YCGE_ERR_INVALID_ARG
    for nv, nt in ((0, 1), (-1, 1), (3, 0), (3, -5)):
        assert fn(pos.ctypes.data, nv, faces.ctypes.data, nt, C.byref(info)) == abi.YCGE_ERR_INVALID_ARG, (nv, nt)
    for bad in (3, -1, 1 << 30):
        f = np.array([[0, 1, bad]], np.int32)
        assert fn(pos.ctypes.data, 3, f.ctypes.data, 1, C.byref(info)) == abi.YCGE_ERR_INVALID_ARG, bad
    assert fn(pos.ctypes.data, 2, faces.ctypes.data, 1, C.byref(info)) == abi.YCGE_ERR_INVALID_ARG          # (index 2 of 2 positions)
    # the context calls refuse a NULL context before anything else
    assert L.ycge_obj_ground(None, C.byref(info)) == abi.YCGE_ERR_INVALID_ARG
    assert L.ycge_obj_triangles_auto_ground(None, 1.0, None, None, None, None) == abi.YCGE_ERR_INVALID_ARG


def test_new_names_are_listed_in_header_abi_bindings_and_hooks(L):
    header = (ROOT / "include" / "ycge.h").read_text()
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text()
    cs = (ROOT / "bindings" / "csharp" / "Ycge.cs").read_text()
    loader = (ROOT / "bindings" / "csharp" / "HipObjLoader.cs").read_text()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\(", header) and name in abi.EXPORTED_SYMBOLS and hasattr(L, name), name
        assert re.search(r"public static extern int " + name + r"\(", cs), name
    for name in NEW_HOOKS:
        assert re.search(r"\bint " + name + r"\(", hooks) and name not in header and hasattr(L, name) and name in abi.OBJ_GROUND_HOOK_PROTOTYPES, name
    assert "typedef struct ycge_obj_ground_info" in header and C.sizeof(abi.ObjGroundInfo) == 64 and "struct YObjGroundInfo" in cs
    assert int(re.search(r"#define YCGE_ABI_VERSION (\d+)", header).group(1)) == 10 == abi.YCGE_ABI_VERSION
    assert "ycge_obj_triangles_auto_ground(" in loader and "Find(" not in loader and "ycge_obj_read(" not in loader          # the private union-find is gone
    from yetanotherconsolegameengine_amd import build
    assert {"ycge_obj.cpp", "ycge_obj_ground.hip"} <= set(build.SOURCES) and {"ycge_obj.h", "ycge_obj_box.hip.h"} <= set(build.HEADERS)
    # the default is the measured crossover, or 0 while nothing is measured
    ctx_h = (CSRC / "ycge_ctx.h").read_text()
    default = int(re.search(r"#define YCGE_OBJ_GROUND_DEVICE_MIN_DEFAULT (\d+)", ctx_h).group(1))
    geo = abi.obj_ground_geometry(L)
    assert geo["device_min_default"] == default and geo["sum_chunk"] > 0 and 2 < geo["round_cap"] <= 64
    rate = ROOT / "profiles" / "obj_ground_rate.json"
    if rate.exists():
        import json
        assert default == json.loads(rate.read_text())["device_min_default"]
    else:
        assert default == 0 and ctx_h.count("NOT YET MEASURED") >= 2


def test_the_cases_hold_what_their_names_say():
    c, w = cases.get("tie_first_has_higher_indices"), want_of("tie_first_has_higher_indices")
    comps = R._components(len(c.pos), c.faces.tolist())
    sizes = sorted(len(v) for v in comps.values())
    assert sizes == [2, 2] and w["first_face"] == 0 and w["component_faces"] == 2
    win = set(c.faces[:2].reshape(-1).tolist())
    lose = set(c.faces[2:].reshape(-1).tolist())
    assert not (win & lose) and min(win) > min(lose)          # the winner is NOT the component of the lowest vertex
    w = want_of("counts_1_2_2")
    assert (w["n_components"], w["component_faces"], w["first_face"]) == (3, 2, 1)
    c, w = cases.get("bridged_by_a_later_face"), want_of("bridged_by_a_later_face")
    assert len(R._components(len(c.pos), c.faces[:-1].tolist())) == 3 and (w["n_components"], w["component_faces"], w["first_face"]) == (2, 7, 0)
    w = want_of("bow_tie")
    assert (w["n_components"], w["component_faces"], w["component_vertices"]) == (2, 8, 11)
    w = want_of("degenerate_and_duplicate")
    assert (w["n_components"], w["component_faces"], w["component_vertices"], w["first_face"]) == (3, 4, 3, 2)
    c, w = cases.get("unnamed_and_losers_outside"), want_of("unnamed_and_losers_outside")
    assert np.abs(w["centroid"]).max() < 1 and w["component_vertices"] == 12 and np.abs(c.pos).max() > 900
    for n in cases.WINNER_SIZES:
        w = want_of(f"winner_{n}")
        assert (w["n_components"], w["component_faces"], w["first_face"]) == (2, n, 2)
    for order in ("ascending", "descending", "shuffled"):
        c, w = cases.get(f"strip_{order}"), want_of(f"strip_{order}")
        assert (w["n_components"], w["component_faces"], w["component_vertices"]) == (1, 1 << 15, (1 << 15) + 2) and len(c.faces) == 1 << 15
    assert cases.get("strip_ascending").faces[0].tolist() == [0, 1, 2] and cases.get("strip_descending").faces[0, 0] == (1 << 15) + 1
    # cancelling: the serial float32 sum is neither numpy's pairwise float32 sum nor the float64 sum rounded once - a tree sum cannot pass
    c, w = cases.get("cancelling"), want_of("cancelling")
    third = np.float32(1.0) / np.float32(3.0)
    terms = ((c.pos[c.faces[:, 0]] + c.pos[c.faces[:, 1]]) + c.pos[c.faces[:, 2]]) * third
    inv = np.float32(1.0) / np.float32(len(c.faces))
    pairwise = np.array([np.sum(np.ascontiguousarray(terms[:, k]), dtype=np.float32) for k in range(3)], np.float32) * inv          # (pairwise along a contiguous vector only)
    once = np.sum(terms.astype(np.float64), axis=0).astype(np.float32) * inv
    differs = [k for k in range(3) if w["centroid"][k] != pairwise[k] and w["centroid"][k] != once[k]]
    assert differs, (w["centroid"], pairwise, once)
    assert np.abs(c.pos).min() > 400 and np.abs(w["centroid"]).max() < 100
    w = want_of("y_extreme_zero")
    assert w["min"][1] == 0 and np.signbit(w["min"][1]) and w["max"][1] == 0 and not np.signbit(w["max"][1]) and w["centroid"][1] == 0
    c, w = cases.get("inf_position"), want_of("inf_position")
    assert b"1e39" in c.text and not c.device_parse and np.isnan(w["centroid"][0]) and np.isfinite(w["centroid"][1:]).all()
    c, w = cases.get("grid_with_islands"), want_of("grid_with_islands")
    assert (w["n_components"], w["component_faces"], w["first_face"]) == (4, 1 << 17, 3) and len(c.faces) == (1 << 17) + 9
    for name in cases.NAMES:          # %.9g stays inside the kernels' exact float domain: 15 digits, a decimal exponent within +-22
        if cases.get(name).device_parse:
            for tok in re.findall(rb"[-+.\deE]+", b" ".join(ln[2:] for ln in cases.get(name).text.split(b"\n")[:2000] if ln.startswith(b"v "))):
                mant, _, ex = tok.lower().partition(b"e")
                digits = mant.lstrip(b"+-").replace(b".", b"")
                frac = len(mant.partition(b".")[2])
                assert len(digits.lstrip(b"0")) <= 15 and abs(int(ex or 0) - frac) <= 22, (name, tok)


PROGRAM = r"""
// the host tail alone, on arrays read from a file: u32 n_cases, then per case i32 n_positions, i32 n_triangles, the floats, the indices
#include "ycge_obj.h"
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t n_cases = 0;
    if (std::fread(&n_cases, 4, 1, f) != 1) return 2;
    for (uint32_t k = 0; k < n_cases; k++) {
        int32_t n[2];
        if (std::fread(n, 4, 2, f) != 2) return 2;
        std::vector<float> pos((size_t)3 * n[0]);
        std::vector<int32_t> faces((size_t)3 * n[1]);
        if (std::fread(pos.data(), 4, pos.size(), f) != pos.size() || std::fread(faces.data(), 4, faces.size(), f) != faces.size()) return 2;
        ycge_obj::GroundInfo g;
        const int rc = ycge_obj::ground_host(pos.data(), n[0], faces.data(), n[1], g);
        uint32_t w[16];
        std::memcpy(w, &g, 64);
        std::printf("%d", rc);
        for (int i = 0; i < 16; i++) std::printf(" %u", w[i]);
        std::printf("\n");
        // refusals leave no read behind them: an index one past the end, a NULL array
        const int32_t keep = faces[0];
        faces[0] = n[0];
        if (ycge_obj::ground_host(pos.data(), n[0], faces.data(), n[1], g) != ycge_obj::ST_INVALID_ARG) return 3;
        faces[0] = keep;
        if (ycge_obj::ground_host(nullptr, n[0], faces.data(), n[1], g) != ycge_obj::ST_INVALID_ARG) return 3;
    }
    std::fclose(f);
    return 0;
}
"""


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/ycge_obj.h stands alone: a program with its own main includes it and runs the host tail over the small cases, compiled with
    -fsanitize=address,undefined and run as a child process (nothing sanitized is loaded into python)."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    names = list(cases.SMALL) + ["strip_shuffled"]
    blob = [np.uint32(len(names)).tobytes()]
    for name in names:
        c = cases.get(name)
        blob += [np.array([len(c.pos), len(c.faces)], np.int32).tobytes(), c.pos.tobytes(), c.faces.tobytes()]
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    (tmp_path / "main.cpp").write_text(PROGRAM)
    exe = tmp_path / "ground_host"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                        str(tmp_path / "main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(names)
    for name, line in zip(names, lines):
        got = [int(t) for t in line.split()]
        assert got[0] == 0 and got[1:15] == want_words(want_of(name)) and got[15:] == [0, 0], name
