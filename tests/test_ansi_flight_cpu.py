"""ANSI streams with frames in flight, the part no GPU is needed for: the export exists, and the two structs of its interface have the
size and the field order include/ycge.h gives them, in the library (ycge_abi_sizeof) and in the ctypes mirror."""
import ctypes as C
import re
from pathlib import Path

from yetanotherconsolegameengine_amd import abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "ycge.h").read_text()


def test_the_library_exports_the_call(product_lib):
    assert hasattr(product_lib, "ycge_render_frame_async_ansi")
    assert "ycge_render_frame_async_ansi" in abi.EXPORTED_SYMBOLS
    assert hasattr(product_lib, "ycge_test_ansi_deliver")
    assert int(re.search(r"#define YCGE_ABI_VERSION (\d+)", HEADER).group(1)) == 10


def test_struct_sizes_in_the_mirror_and_in_the_library(product_lib):
    assert C.sizeof(abi.AnsiAsync) == 48
    assert C.sizeof(abi.AnsiAsyncResult) == 32
    product_lib.ycge_abi_sizeof.restype = C.c_size_t
    product_lib.ycge_abi_sizeof.argtypes = [C.c_int32]
    assert product_lib.ycge_abi_sizeof(abi.ABI_SIZEOF_ANSI_ASYNC) == C.sizeof(abi.AnsiAsync)
    assert product_lib.ycge_abi_sizeof(abi.ABI_SIZEOF_ANSI_ASYNC_RESULT) == C.sizeof(abi.AnsiAsyncResult)
    assert (abi.ABI_SIZEOF_ANSI_ASYNC, abi.ABI_SIZEOF_ANSI_ASYNC_RESULT) == (12, 13)
    assert product_lib.ycge_abi_sizeof(14) == 0          # (the two are the last)


def header_fields(name):
    """[(field, C type, count)] of `typedef struct name { ... } name;` in the header, comments removed"""
    body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + r";", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        ctype, names = stmt.split(None, 1)
        for n in names.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", n.strip())
            out.append((m.group(1), ctype, int(m.group(2) or 1)))
    return out


CTYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}


def test_field_order_of_the_header_is_the_mirrors():
    for name, twin in (("ycge_ansi_async", abi.AnsiAsync), ("ycge_ansi_async_result", abi.AnsiAsyncResult)):
        fields = header_fields(name)
        assert [f[0] for f in fields] == [f[0] for f in twin._fields_], name
        for (fname, ctype, count), (_, t) in zip(fields, twin._fields_):
            want = CTYPES[ctype] * count if count > 1 else CTYPES[ctype]
            assert C.sizeof(t) == C.sizeof(want) and (t is want or (count > 1 and t._type_ is CTYPES[ctype] and t._length_ == count)), (name, fname)
    assert abi.AnsiAsyncResult.length.offset == 0 and abi.AnsiAsyncResult.info.offset == 8
    assert abi.AnsiAsyncResult.status.offset == 24 and abi.AnsiAsyncResult.reserved.offset == 28


def test_prototypes_of_the_call_and_its_hook():
    res, args = abi._PROTOTYPES["ycge_render_frame_async_ansi"]
    assert res is C.c_int and len(args) == 6
    res, args = abi.ANSI_FLIGHT_HOOK_PROTOTYPES["ycge_test_ansi_deliver"]
    assert res is C.c_int and len(args) == 10
