"""ycge_obj_parse_host - the library's host OBJ parser, the yardstick and fallback of the device parse - against tests/obj_restatement.py,
bit for bit (uint32 views of the floats; no tolerance anywhere).  No GPU is touched: the device side is tests/test_gpu_obj.py."""
import ctypes as C
import os
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import obj_cases
import obj_restatement as R
from yetanotherconsolegameengine_amd import abi, mesh_loader

ROOT = Path(__file__).resolve().parents[1]
NEW_EXPORTS = ("ycge_obj_parse_host", "ycge_obj_parse", "ycge_obj_read", "ycge_obj_triangles", "ycge_obj_release")


@pytest.fixture(scope="module")
def L():
    lib = abi.load_library()
    for name in NEW_EXPORTS:
        fn = getattr(lib, name)          # (AttributeError - a failure, not a skip - when the export is missing)
        fn.restype, fn.argtypes = abi._PROTOTYPES[name]
    return lib


def host(L, data):
    pos, faces, info = abi.obj_parse_host(data, L)
    return pos, faces, info


def refusal_of(message: str):
    m = re.search(r"OBJ line (\d+):", message)
    if m:
        return "line", int(m.group(1))
    m = re.search(r"OBJ triangle (\d+) ", message)
    if m:
        return "triangle", int(m.group(1))
    return ("none", None) if "no position or no triangle" in message else ("?", None)


@pytest.mark.parametrize("name", sorted(obj_cases.CASES))
def test_host_parser_equals_the_restatement(L, name):
    data, _ = obj_cases.CASES[name]
    want_pos, want_faces, want_lines = R.parse(data)
    pos, faces, info = host(L, data)
    assert (info.n_positions, info.n_triangles, info.n_lines, info.on_device) == (len(want_pos), len(want_faces), want_lines, 0)
    assert np.array_equal(pos.view(np.uint32), want_pos), name
    assert np.array_equal(faces, want_faces), name


def test_the_cases_hold_what_their_names_say():
    """the inputs themselves: the terminators, separators and forms the issue lists are really in them"""
    mixed = obj_cases.CASES["drawn_mixed_0"][0]
    assert b"\r\n" in mixed and re.search(rb"[^\r]\n", mixed) and re.search(rb"\r[^\n]", mixed)
    assert all(s in mixed for s in (b"\t", b"\x0b", b"\x0c", b"\x1f", b" # x", b"--1e", b"caf\xc3\xa9"))
    _, faces, _ = R.parse(obj_cases.CASES["faces_3_to_8"][0])
    assert len(faces) == sum(n - 2 for n in range(3, 9))
    assert not obj_cases.CASES["no_final_terminator"][0].endswith((b"\n", b"\r")) and obj_cases.CASES["lone_cr_last_byte"][0].endswith(b"3\r")
    # .NET does not split at 0x1F, Python's str.split does: the restatement follows .NET
    sep = obj_cases.CASES["separators"][0]
    pos, faces, _ = R.parse(sep)
    assert faces.tolist() == [[0, 1, 2]]
    assert len(sep.decode("latin-1").split("\n")[3].split()) == 5          # str.split: f, 1/9, 8, 2, 3


def test_float_forms_known_answers(L):
    def one(tok):
        pos, _, _ = host(L, b"v " + tok + b" 1 1\nf 1 1 1\n")
        assert pos.view(np.uint32)[0, 0] == R.float_bits(tok), tok
        return pos[0, 0]

    assert one(b"+1") == 1 and one(b".5") == 0.5 and one(b"5.") == 5 and one(b"1e-3") == np.float32(0.001) and one(b"1E+05") == 100000
    z = one(b"-0")
    assert z == 0 and np.signbit(z)
    assert one(b"16777217") == 16777216 and one(b"16777219") == 16777220          # exact midpoints: ties to even
    assert one(b"12345678901234567890") == np.float32(1.2345679e19)
    assert one(b"1e39") == np.inf and one(b"-1e39") == -np.inf and one(b"3.4028235e38") == np.finfo(np.float32).max
    sub = one(b"1e-45")
    assert sub.view(np.uint32) == 1 and one(b"0.7e-45") == 0 and one(b"1e-400") == 0
    assert one(b"1.17549421e-38").view(np.uint32) == 0x007FFFFF          # the largest subnormal


def test_double_rounding_witness_goes_wrong_by_way_of_binary64(L):
    """at least one decimal on which decimal -> binary64 -> binary32 differs from the correct rounding: a 20-digit neighbour of the midpoint
    1 + 2^-24.  (It is outside the device's 15-digit domain by design: the host parser reads such files.)"""
    tok = b"1.0000000596046447754"
    assert Fraction(tok.decode()) > 1 + Fraction(1, 1 << 24)
    via_double = np.float32(float(tok)).view(np.uint32)
    correct = R.float_bits(tok)
    assert via_double == 0x3F800000 and correct == 0x3F800001
    pos, _, _ = host(L, obj_cases.CASES["double_rounding_witness"][0])
    assert pos.view(np.uint32)[0, 0] == correct
    lines = obj_cases.CASES["double_rounding_witness"][0].decode().splitlines()
    ml, _ = mesh_loader.parse_obj(lines)
    assert ml.view(np.uint32)[0, 0] == via_double          # mesh_loader.parse_obj rounds twice (it stays as it is)


def test_double_rounding_witnesses_exist_inside_the_device_domain(L):
    """The search the device's float routine was written against: 14- and 15-digit decimals printed beside drawn binary32 midpoints.  About
    one in a thousand of them rounds differently by way of binary64,
    so the remainder branch of the kernels' routine is live inside its 15-digit domain; five of them are pinned here and in
    obj_cases.CASES["midpoint_neighbours"], which the device must parse itself."""
    data = obj_cases.CASES["midpoint_neighbours"][0]
    toks = [t for line in data.split(b"\n")[:2] for t in line.split()[1:]]
    assert len(toks) == 6
    for tok in toks:
        assert len(tok.lstrip(b"-").split(b"e")[0].replace(b".", b"")) <= 15
        assert np.float32(float(tok)).view(np.uint32) != R.float_bits(tok), tok
    pos, _, _ = host(L, data)
    assert [int(b) for b in pos.view(np.uint32)[:2].reshape(-1)] == [R.float_bits(t) for t in toks]


@pytest.mark.parametrize("name", sorted(obj_cases.REFUSALS))
def test_refusals_with_precedence_and_the_line_or_triangle_named(L, name):
    data, status, kind, number = obj_cases.REFUSALS[name]
    with pytest.raises(R.Refusal) as want:
        R.parse(data)
    assert (want.value.status, want.value.kind, want.value.number) == (status, kind, number)
    with pytest.raises(abi.YcgeError) as got:
        host(L, data)
    assert got.value.status == status
    assert refusal_of(str(got.value)) == (kind, number), str(got.value)


def test_argument_refusals_message_buffer_and_counts_only(L):
    info, msg = abi.ObjInfo(), C.create_string_buffer(256)
    fn = L.ycge_obj_parse_host
    assert fn(None, 10, None, None, C.byref(info), msg, 256) == abi.YCGE_ERR_INVALID_ARG and b"NULL or empty" in msg.value
    assert fn(b"", 0, None, None, C.byref(info), msg, 256) == abi.YCGE_ERR_INVALID_ARG
    assert fn(b"v", 1 << 31, None, None, C.byref(info), msg, 256) == abi.YCGE_ERR_INVALID_ARG and b"2^31" in msg.value          # (refused before a byte is read)
    assert fn(obj_cases.TRI, len(obj_cases.TRI), None, None, None, msg, 256) == abi.YCGE_ERR_INVALID_ARG
    # a msg buffer of 1 byte holds the terminator and nothing is written behind it; no buffer at all is fine too
    small = (C.c_char * 4)(b"\x7f", b"\x7f", b"\x7f", b"\x7f")
    bad = obj_cases.REFUSALS["bad_float"][0]
    assert fn(bad, len(bad), None, None, C.byref(info), small, 1) == abi.YCGE_ERR_INVALID_ARG and small.raw == b"\x00\x7f\x7f\x7f"
    assert fn(bad, len(bad), None, None, C.byref(info), None, 0) == abi.YCGE_ERR_INVALID_ARG
    assert (info.n_positions, info.n_triangles, info.n_lines) == (0, 0, 0)
    # counts only
    data = obj_cases.CASES["drawn_mixed_0"][0]
    want_pos, want_faces, want_lines = R.parse(data)
    assert fn(data, len(data), None, None, C.byref(info), None, 0) == abi.YCGE_OK
    assert (info.n_positions, info.n_triangles, info.n_lines) == (len(want_pos), len(want_faces), want_lines)
    # one array only
    faces = np.full((info.n_triangles, 3), -7, np.int32)
    assert fn(data, len(data), None, faces.ctypes.data, C.byref(info), None, 0) == abi.YCGE_OK and np.array_equal(faces, want_faces)


@pytest.mark.parametrize("name", ["suite_forms", "drawn_plain", "faces_3_to_8", "crlf", "v_3_and_7_tokens"])
def test_tail_agrees_with_mesh_loader_where_parse_obj_is_exact(L, name):
    """mesh_loader.parse_obj reads these files as the reference does (no 0x1F-split difference reaches a parsed token, every float survives
    its double rounding): the three parsers agree, and the restated tail equals mesh_loader.from_obj_arrays bit for bit."""
    data, _ = obj_cases.CASES[name]
    pos, faces, _ = host(L, data)
    ml_pos, ml_faces = mesh_loader.parse_obj(re.split(r"\r\n|\n|\r", data.decode("latin-1")))
    assert np.array_equal(ml_pos.view(np.uint32), pos.view(np.uint32)) and np.array_equal(ml_faces, faces)
    for kw in (dict(normalize=True, target_size=1.0, scale=1.0, translate=(0.0, 0.0, 0.0)), dict(normalize=False, target_size=1.0, scale=1.0, translate=(0.0, 0.0, 0.0)),
               dict(normalize=True, target_size=2.5, scale=0.75, translate=(1.5, -2.0, 0.25))):
        tris, bounds = R.triangles(pos.view(np.uint32), faces, **kw)
        want = mesh_loader.from_obj_arrays(pos, faces, **kw)
        assert np.array_equal(tris.view(np.uint32), want.view(np.uint32)), (name, kw)
        p = want.reshape(-1, 3)
        assert np.array_equal(bounds, np.concatenate([p.min(0), p.max(0)]))


def test_new_names_are_listed_in_header_abi_and_hooks(L):
    header = (ROOT / "include" / "ycge.h").read_text()
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\(", header) and name in abi.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert "typedef struct ycge_obj_info" in header and C.sizeof(abi.ObjInfo) == 24
    assert re.search(r"\bint ycge_debug_obj_stats\(", hooks) and "ycge_debug_obj_stats" not in header and hasattr(L, "ycge_debug_obj_stats")
    assert int(re.search(r"#define YCGE_ABI_VERSION (\d+)", header).group(1)) == 10
    geo = abi.obj_geometry(L)
    ctx_h = (ROOT / "yetanotherconsolegameengine_amd" / "csrc" / "ycge_ctx.h").read_text()
    default = int(re.search(r"#define YCGE_OBJ_DEVICE_MIN_DEFAULT (\d+)", ctx_h).group(1))
    assert geo["tile_bytes"] > 0 and geo["lines_per_workgroup"] > 0 and geo["line_cap"] >= 256
    if "YCGE_OBJ_DEVICE_MIN" not in os.environ:
        assert geo["device_min"] == default
    rate = ROOT / "profiles" / "obj_rate.json"          # the default is the measured crossover, or 0 while nothing is measured
    if rate.exists():
        import json
        assert default == (json.loads(rate.read_text())["crossover_bytes"] or 0)
    else:
        assert default == 0 and "NOT YET MEASURED" in ctx_h
    from yetanotherconsolegameengine_amd import build
    assert {"ycge_obj.cpp", "ycge_obj.hip"} <= set(build.SOURCES) and "ycge_obj.h" in build.HEADERS
