"""CPU-only tests of the scene queries (ycge_scene_hit / ycge_scene_occluded, ABI 10): the boundary without a device, the exception barrier of
their host file, the C# binding's calls, the Python mirror's ray packing.  The answers themselves are tests/test_gpu_scene_queries.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "yetanotherconsolegameengine_amd" / "csrc"
CS = ROOT / "bindings" / "csharp"


def test_both_exports_refuse_a_null_context_without_a_gpu(product_lib):
    L = product_lib
    rays = np.zeros((1, 8), np.float32); rays[0, 3] = 1.0
    hits = np.zeros((1, 10), np.float32); ids = np.zeros((1, 2), np.int32); occ = np.zeros(1, np.uint8)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.ycge_scene_hit(None, fp(rays), 1, fp(hits), ids.ctypes.data_as(C.POINTER(C.c_int32))) == abi.YCGE_ERR_INVALID_ARG
    assert L.ycge_scene_occluded(None, fp(rays), 1, occ.ctypes.data_as(C.POINTER(C.c_uint8))) == abi.YCGE_ERR_INVALID_ARG
    assert L.ycge_scene_hit(None, None, 0, None, None) == abi.YCGE_ERR_INVALID_ARG
    assert "ycge_scene_hit" in abi.EXPORTED_SYMBOLS and "ycge_scene_occluded" in abi.EXPORTED_SYMBOLS and abi.YCGE_ABI_VERSION == 10


def test_every_export_of_the_query_host_file_is_guarded():
    """the structural rule of test_host_cpu.py::test_every_export_of_the_host_sources_is_guarded, applied to csrc/ycge_query.cpp: every
    function defined in its extern "C" block is a function-try-block whose handler calls abi_catch"""
    lines = (CSRC / "ycge_query.cpp").read_text().split("\n")
    in_c, names = False, []
    for i, line in enumerate(lines):
        if line.startswith('extern "C" {'): in_c = True
        if line.startswith('} // extern "C"'): in_c = False
        m = re.match(r"^(int|size_t|void|const char \*)\s*(ycge_\w+)\(", line) if in_c else None
        if not m or line.rstrip().endswith(";"):
            continue
        j = i
        while lines[j] not in ("try {", "{") and j < i + 6: j += 1
        assert lines[j] == "try {", f"ycge_query.cpp:{i + 1} {m.group(2)} is not a function-try-block"
        k = j + 1
        while lines[k] != "}": k += 1
        assert lines[k + 1].startswith("catch (...) {") and "abi_catch(" in lines[k + 1], f"ycge_query.cpp:{k + 2} {m.group(2)}"
        names.append(m.group(2))
    assert sorted(names) == ["ycge_scene_hit", "ycge_scene_occluded"], names


def _split_args(s):
    """top-level comma split of a call's argument text"""
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "([{": depth += 1
        if ch in ")]}": depth -= 1
        if ch == "," and depth == 0:
            out.append(cur); cur = ""
        else:
            cur += ch
    if cur.strip(): out.append(cur)
    return [a for a in out if a.strip()]


def _calls(src, name_re):
    """(name, [args]) of every call `Ycge.<name>(...)` with balanced parentheses"""
    for m in re.finditer(r"Ycge\.(" + name_re + r")\(", src):
        i, depth = m.end(), 1
        j = i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0)
            j += 1
        yield m.group(1), _split_args(src[i:j - 1])


def test_csharp_scene_query_calls_name_declared_imports():
    """every Ycge.ycge_* call in HipSceneQuery.cs names a [DllImport] of Ycge.cs and passes its declared number of arguments"""
    ycge = (CS / "Ycge.cs").read_text()
    imports = {m.group(1): len([p for p in m.group(2).split(",") if p.strip()])
               for m in re.finditer(r"\[DllImport\(Lib\)\]\s*public static extern \w+ (ycge_\w+)\(([^)]*)\);", ycge)}
    src = (CS / "HipSceneQuery.cs").read_text()
    calls = list(_calls(src, r"ycge_\w+"))
    assert {n for n, _ in calls} == {"ycge_scene_hit", "ycge_scene_occluded"}, calls
    for name, args in calls:
        assert name in imports, name
        assert len(args) == imports[name], (name, args, imports[name])
        assert len(args) == len(abi._PROTOTYPES[name][1]), name
    # and the wrapper hands the queries its context through the accessor
    wrapper = (CS / "HipRaytraceWrapper.cs").read_text()
    assert "internal IntPtr NativeContext => ctx;" in wrapper and "new HipSceneQuery(" in wrapper


def test_python_mirror_packs_rays_and_broadcasts_the_interval():
    o = np.arange(12, dtype=np.float64).reshape(4, 3)
    d = -np.arange(12, dtype=np.float64).reshape(4, 3) - 1
    r = RaytraceRenderer._query_rays(o, d, 0.5, np.array([1, 2, 3, np.inf]))
    assert r.dtype == np.float32 and r.shape == (4, 8) and r.flags["C_CONTIGUOUS"]
    assert np.array_equal(r[:, 0:3], o.astype(np.float32)) and np.array_equal(r[:, 3:6], d.astype(np.float32))
    assert (r[:, 6] == np.float32(0.5)).all() and np.array_equal(r[:, 7], np.array([1, 2, 3, np.inf], np.float32))
    assert RaytraceRenderer._query_rays([0, 0, 0], [0, 0, 1], 0.001, 10.0).shape == (1, 8)
