"""No GPU: the pool of materialised chunks beside a fields-form world store (ycge_world_store_reserve_edits / _edit_slots / _revert_chunks)
is declared alike in include/ycge.h, abi.py and the C# binding, and the refusals that need no device."""
import ctypes as C
import re
from pathlib import Path

import pytest

from yetanotherconsolegameengine_amd import abi

ROOT = Path(__file__).resolve().parents[1]

# name -> the C parameter types of the header, in order; what each is in abi.py and in Ycge.cs
EXPORTS = {
    "ycge_world_store_reserve_edits": ["ycge_ctx *", "int32_t"],
    "ycge_world_store_edit_slots": ["ycge_ctx *", "int32_t *", "int32_t *"],
    "ycge_world_store_revert_chunks": ["ycge_ctx *", "const int32_t *", "int32_t"],
}
CTYPES = {"ycge_ctx *": C.c_void_p, "int32_t": C.c_int32, "int32_t *": C.POINTER(C.c_int32), "const int32_t *": C.POINTER(C.c_int32)}
CSHARP = {"ycge_ctx *": "IntPtr", "int32_t": "int", "int32_t *": "int*", "const int32_t *": "int*"}


def _c_params(text, name):
    m = re.search(r"^int " + name + r"\(([^)]*)\);", text, re.M)
    assert m, name
    params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).split(",")]
    return [re.sub(r"\s*\w+$", "", p).strip() for p in params]          # the type: the declaration without the parameter's name


def test_header_abi_and_csharp_declare_the_same_signatures():
    header, hooks = (ROOT / "include" / "ycge.h").read_text(), (ROOT / "include" / "ycge_hooks.h").read_text()
    cs, cs_world = (ROOT / "bindings" / "csharp" / "Ycge.cs").read_text(), (ROOT / "bindings" / "csharp" / "YcgeWorld.cs").read_text()
    for name, want in EXPORTS.items():
        assert _c_params(header, name) == want, name
        assert ("int " + name + "(") not in hooks and name in abi.EXPORTED_SYMBOLS
        res, args = abi._PROTOTYPES[name]
        assert res is C.c_int and args == [CTYPES[t] for t in want], name
        m = re.search(r"\[DllImport\(Lib\)\] public static extern int " + name + r"\(([^)]*)\);", cs)
        assert m, name
        assert [p.strip().rsplit(" ", 1)[0] for p in m.group(1).split(",")] == [CSHARP[t] for t in want], name
        assert ("Ycge." + name + "(") in cs_world, name
    for method in ("public void ReserveEdits(IntPtr ctx, int maxChunks)", "public int[] EditSlots(IntPtr ctx)", "public void RevertChunks(IntPtr ctx, int[] keys)"):
        assert method in cs_world, method
    assert abi.YCGE_ABI_VERSION == 10 and re.search(r"#define\s+YCGE_ABI_VERSION\s+10\b", header)


def test_the_header_states_the_pool_s_cost_and_rules():
    header = re.sub(r"\s*\n \*\s*", " ", (ROOT / "include" / "ycge.h").read_text())
    for text in ("max_chunks * S^3 * 8 bytes", "EVERY CHUNK AN OP TOUCHES TAKES A SLOT", "two ways to run out of slots", "ycge_world_store_revert_chunks"):
        assert text in header, text


def test_the_layers_above_carry_the_pool():
    import inspect
    from yetanotherconsolegameengine_amd import world_file
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    for method in ("ReserveWorldEdits", "WorldEditSlots", "RevertWorldChunks"):
        assert callable(getattr(RaytraceRenderer, method)), method
    assert "edit_chunks" in inspect.signature(world_file.pregen_resident).parameters


def test_refusals_that_need_no_device():
    try:
        L = abi.load_library()
    except OSError as e:
        pytest.skip(f"the library does not load here: {e}")
    cap, used = C.c_int32(7), C.c_int32(7)
    key = (C.c_int32 * 3)(0, 0, 0)
    assert L.ycge_world_store_reserve_edits(None, 4) == abi.YCGE_ERR_INVALID_ARG
    assert L.ycge_world_store_edit_slots(None, C.byref(cap), C.byref(used)) == abi.YCGE_ERR_INVALID_ARG and (cap.value, used.value) == (7, 7)
    assert L.ycge_world_store_revert_chunks(None, key, 1) == abi.YCGE_ERR_INVALID_ARG
