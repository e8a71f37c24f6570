"""OBJ texts shared by tests/test_obj_cpu.py and tests/test_gpu_obj.py: {name: (bytes, in_device_domain)}.

in_device_domain: every float token has at most 15 significant digits and a decimal exponent within +-22 once its fraction digits are
counted in, and no line that is not a comment is longer than the kernels' line cap - the device must parse such a file itself.
Drawn coordinates are never zero, so no extreme of a drawn file is a signed zero (include/ycge.h: the one thing the reference leaves to
HashSet enumeration order)."""
from __future__ import annotations

import random

# the forms the suite already uses (tests/test_host_cpu.py::test_obj_subset_parser) plus a pentagon
OBJ_TEXT = b"""# comment
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0

f 1/1/1 2/2/2 3/3/3 4/4/4
v 0 0 1
f -1 -2 -3
f 1// 2// 5//
v 0.5 1.5 0.25
f 1 2 3 4 6
"""

# the small hull of tests/test_gpu_timed_variants.py::test_scene_loaded_from_obj_text_against_oracle: every index form, quads, a pentagon
HULL = b"""# a small hull with every index form MeshLoader.cs:23-55 accepts
v -0.6 0.0 -0.4
v 0.6 0.0 -0.4
v 0.6 0.0 0.4
v -0.6 0.0 0.4
v 0.0 0.9 0.0
vt 0 0
vn 0 1 0
f 1 2 3 4
f 1/1/1 2/1/1 5/1/1
f 2//1 3//1 5//1
f -3 -2 -1
f 4 1 5
v 0.0 -0.5 0.0
f 1 2 3 4 6
f -1 -3 -5 -6
"""

SEPS = [b" ", b"\t", b"\x0b", b"\x0c", b"  ", b" \t "]
ENDS = [b"\n", b"\r\n", b"\r"]


def _coord(rng: random.Random) -> bytes:
    x = rng.uniform(0.001, 10.0) * rng.choice((-1, 1))
    form = rng.randrange(6)
    if form == 0:
        return b"%.6f" % x
    if form == 1:
        return b"%.3e" % x
    if form == 2:
        return b"%.9g" % x
    if form == 3:
        return (b"+" if x > 0 else b"") + b"%.2f" % x
    if form == 4:
        return b"%dE+0%d" % (rng.randrange(1, 99) * rng.choice((-1, 1)), rng.randrange(0, 3))
    return (b"-" if x < 0 else b"") + b".%d" % rng.randrange(1, 99999)


def drawn(seed: int, n_lines: int = 300, ends=None, n_face_max: int = 8, only_negative: bool = False, comments: bool = True, x1f: bool = True) -> bytes:
    """a file of n_lines lines: v lines (3-token, 4-token, 7-token with garbage), f lines of 3..n_face_max corners in every index form with
    forward references, comments with bytes >= 0x80, " # x" lines, other keywords, empty lines; mixed terminators and separators"""
    rng = random.Random(seed)
    ends = ends or ENDS
    kinds = []
    for _ in range(n_lines):
        r = rng.random()
        kinds.append("v" if r < 0.40 else "f" if r < 0.80 else "x")
    kinds[0] = "v"
    nv = kinds.count("v")
    out, count = [], 0
    for kind in kinds:
        sep = lambda: rng.choice(SEPS)
        if kind == "v":
            line = b"v" + b"".join(sep() + _coord(rng) for _ in range(3))
            if rng.random() < 0.15:
                line += sep() + b"1.0" + sep() + b"ga,rb/age" + sep() + b"--1e"          # 7 tokens: the extras are never parsed
            count += 1
        elif kind == "f":
            corners = []
            for _ in range(rng.randrange(3, n_face_max + 1)):
                form = 1 if only_negative else rng.randrange(5)
                if form == 0:
                    i = rng.randrange(1, nv + 1)                       # any vertex of the file: forward references
                elif form == 1 and count > 0:
                    i = -rng.randrange(1, count + 1)
                elif form == 2 and count < nv:
                    i = 0                                               # count + 0: the vertex the NEXT v line defines
                else:
                    i = rng.randrange(1, nv + 1)
                tail = rng.choice((b"", b"/3", b"/3/4", b"//4", b"/", b"/x\x1fy" if x1f else b"/xy"))
                corners.append(b"%d" % i + tail)
            line = (b"" if rng.random() < 0.9 else b" ") + b"f" + b"".join(sep() + c for c in corners)
            if rng.random() < 0.2:
                line += sep()
        else:
            r = rng.randrange(7 if comments else 6)
            line = [b"", b" # x", b"vn 0 0 1", b"v 1 2", b"usemtl a\x1fb", b"\t", b"# caf\xc3\xa9 \xff"][r]
        out.append(line + rng.choice(ends))
    text = b"".join(out)
    if seed & 1:
        text = text.rstrip(b"\r\n") or text                            # a last line without a terminator
    return text


def padded_to(text: bytes, size: int) -> bytes:
    """`text` behind a leading comment line that brings the file to exactly `size` bytes"""
    need = size - len(text)
    assert need >= 2, (need, size)
    return b"#" + b"p" * (need - 2) + b"\n" + text


TRI = b"v 1 2 3\nv -4 5 6\nv 7 -8 9\nf 1 2 3\n"


def at_offset(text: bytes, offset: int) -> bytes:
    """`text` starting at byte `offset`, behind one comment line"""
    assert offset >= 2
    return b"#" + b"o" * (offset - 2) + b"\n" + text


def n_lines_file(k: int) -> bytes:
    """exactly k lines: k - 1 `v` lines and one face at the end (k = 1: the face alone - refused, it names no position)"""
    return b"".join(b"v %d.5 -%d.25 %d\n" % (j % 97, j % 13 + 1, j % 7 + 1) for j in range(k - 1)) + b"f 1 -1 %d" % max(1, (k - 1) // 2)


def many_lines_file(n: int = 66000) -> bytes:
    """n short lines, about 1.1 MB: more tiles of text and more workgroups of lines than the one-workgroup scans take in one trip"""
    lines = [b"v %d.5 -%d.25 %d.125" % (k % 97, k % 13, k % 7) if (k % 3 or k < 3) else b"f %d %d -1" % (1, max(1, k // 3)) for k in range(n - 1)]
    return b"\n".join(lines + [b"f 1 2 3"]) + b"\n"


def ngon_line(line_bytes: int) -> bytes:
    """three positions and one `f` line of exactly line_bytes bytes (separators at its end make up the length)"""
    corners = (line_bytes - 1) // 2
    line = b"f" + b"".join(b" %d" % (j % 3 + 1) for j in range(corners))
    return b"v 1 2 3\nv -4 5 6\nv 7 -8 9\n" + line + b" " * (line_bytes - len(line)) + b"\n"

CASES = {
    "suite_forms": (OBJ_TEXT, True),
    "hull": (HULL, True),
    "drawn_mixed_0": (drawn(10), True),
    "drawn_mixed_1": (drawn(11), True),
    "drawn_mixed_2": (drawn(12, n_lines=700), True),
    "drawn_plain": (drawn(15, x1f=False), True),                       # no 0x1F inside a corner token: Python's str.split reads it as .NET does
    "bom": (b"\xef\xbb\xbf" + drawn(13, n_lines=40), True),
    "bom_then_comment": (b"\xef\xbb\xbf# only\n" + TRI, True),
    "separators": (b"v\t1\x0b2\x0c3\nv \t 4 \x0b\x0c 5  6\t\nv 7 8 9\nf\t1/9\x1f8 2\x0b3\n", True),            # 0x1F is inside a token (str.split would cut there)
    "no_final_terminator": (TRI.rstrip(b"\n"), True),
    "lone_cr_last_byte": (TRI.replace(b"\n", b"\r"), True),
    "crlf": (TRI.replace(b"\n", b"\r\n"), True),
    "cr_cr_lf": (b"v 1 2 3\r\r\nv -4 5 6\n\rv 7 -8 9\r\n\r\nf 1 2 3\r", True),
    "comments_high_bytes": (b"# \xe9\xff\x80\n" + TRI + b"#\xf0\x9f\x98\x80", True),
    "space_hash_lines": (b" # x\n" + TRI + b" # v 1 2 3\n\t#f 1 2 3\n", True),
    "v_3_and_7_tokens": (b"v 1 2\n" + TRI + b"v 9 8 7 1.0 xx yy,zz\nv 1\nv\nf 4 2 1\n", True),
    "faces_3_to_8": (b"".join(b"v %d %d %d\n" % (k + 1, 2 * k - 5, 7 - k * k) for k in range(8)) + b"".join(b"f " + b" ".join(b"%d" % (j + 1) for j in range(n)) + b"\n" for n in range(3, 9)) + b"f 1 2\nf 1\nf\n", True),
    "forward_references": (b"f 1 2 3\nf -0 1 2\nv 1 2 3\nf 0 -1 3\nv -4 5 6\nv 7 -8 9\n", True),
    "float_forms": (b"v +1 .5 5.\nv -0 1e-3 1E+05\nv 16777217 16777219 -16777217\nv 0.000 -0.0e5 00012.50\nv 123456789012345 1e22 1e-22\nv 9.99999999999999e22 0.1 1.17549435e-14\nf 1 2 3 4 5 6\n", True),
    # 14- and 15-digit neighbours of binary32 midpoints on which binary64-then-binary32 rounds the wrong way: INSIDE the kernels' domain
    # (found by a search beside drawn midpoints), so the device's exact-remainder branch runs, both for the multiply and for the divide
    "midpoint_neighbours": (b"v 3.22335037878934e+34 2.6194141676911e+24 5.14619896421209e-04\nv 1.92815400660038e-01 4.05680920112822e+33 -5.14619896421209e-04\nv 1 2 3\nf 1 2 3\n", True),
    "all_negative": (drawn(14, n_lines=120, only_negative=True), True),
    # host domain: the device declines these files as a whole
    "float_forms_host": (b"v 12345678901234567890 0.12345678901234567890 1e-45\nv 1e39 -1e39 1e-60\nv 1.4e-45 3.4028235e38 3.4028236e38\nv 1e-400 1e400 0.7e-45\nf 1 2 3 4\n", False),
    "double_rounding_witness": (b"v 1.0000000596046447754 2 3\nv 1.00000005960464477539 5 6\nv 7 8 1.0000000596046447753\nf 1 2 3\n", False),
    "sixteen_digits": (b"v 1.234567890123456 2 3\nv 4 5 6\nv 7 8 9\nf 1 2 3\n", False),
    "exponent_23": (b"v 1e23 2 3\nv 4 5 6\nv 7 8 9\nf 1 2 3\n", False),
    "exponent_minus_23": (b"v 0.1e-22 2 3\nv 4 5 6\nv 7 8 9\nf 1 2 3\n", False),
}

# (text, status, kind, number): every refusal, with the line or triangle it names
INVALID_ARG, UNSUPPORTED = -1, -4
REFUSALS = {
    "bad_float": (b"v 1 2 3\nv 1 2 x\nf 1 1 1\n", INVALID_ARG, "line", 2),
    "bad_float_forms": (b"v 1 2 3\n\nv 1,000 2 3\nf 1 1 1\n", INVALID_ARG, "line", 3),
    "infinity_word": (b"v Infinity 2 3\nf 1 1 1\n", INVALID_ARG, "line", 1),
    "nan_word": (b"v 1 NaN 3\nf 1 1 1\n", INVALID_ARG, "line", 1),
    "lone_dot": (b"v . 2 3\nf 1 1 1\n", INVALID_ARG, "line", 1),
    "exponent_without_digits": (b"v 1e 2 3\nf 1 1 1\n", INVALID_ARG, "line", 1),
    "hex_float": (b"v 0x10 2 3\nf 1 1 1\n", INVALID_ARG, "line", 1),
    "bad_int": (b"v 1 2 3\nf 1 1 1x\n", INVALID_ARG, "line", 2),
    "int_is_float": (b"v 1 2 3\nf 1 1.0 1\n", INVALID_ARG, "line", 2),
    "int_overflow": (b"v 1 2 3\nf 1 1 2147483648\n", INVALID_ARG, "line", 2),
    "int_sign_only": (b"v 1 2 3\nf 1 - 1\n", INVALID_ARG, "line", 2),
    "two_bad_lines": (b"v 1 2 3\n" * 5 + b"f 1 2 q\n" + b"v 1 2 3\n" * 2000 + b"v 1 2 z\nf 1 1 1\n", INVALID_ARG, "line", 6),            # (the second one lies in another tile)
    "two_bad_lines_far": (b"v 1 2 3\n" * 3000 + b"v a 2 3\n" + b"v 1 2 3\n" * 3000 + b"f 1 2 q\n", INVALID_ARG, "line", 3001),
    "non_ascii_line": (b"v 1 2 3\no caf\xc3\xa9\nf 1 1 1\n", UNSUPPORTED, "line", 2),
    "non_ascii_before_bad_token": (b"v 1 2 3\nv 1 2 \xa0 3\nv 1 2 x\nf 1 1 1\n", UNSUPPORTED, "line", 2),
    "bad_token_before_non_ascii": (b"v 1 2 x\nv 1 2 \xa0 3\nf 1 1 1\n", INVALID_ARG, "line", 1),
    "non_ascii_on_the_bad_line": (b"v 1 2 x \xff\nf 1 1 1\n", UNSUPPORTED, "line", 1),
    "bad_token_beats_no_triangle": (b"v 1 2 x\n", INVALID_ARG, "line", 1),
    "bad_token_beats_range": (b"v 1 2 3\nf 1 2 3\nf 1 1 z\n", INVALID_ARG, "line", 3),
    "no_position": (b"f 1 2 3\n", INVALID_ARG, "none", None),
    "no_triangle": (b"v 1 2 3\nf 1 2\n", INVALID_ARG, "none", None),
    "only_comments": (b"# nothing\n\n", INVALID_ARG, "none", None),
    "only_bom": (b"\xef\xbb\xbf", INVALID_ARG, "none", None),
    "none_beats_range": (b"f 1 2 3\nf 4 5 6\n", INVALID_ARG, "none", None),
    "index_too_large": (b"v 1 2 3\nv 4 5 6\nf 1 2 1\nf 1 2 3 1\nf 9 9 9\n", INVALID_ARG, "triangle", 1),
    "index_negative": (b"v 1 2 3\nf 1 1 1\nf -2 1 1\nv 4 5 6\n", INVALID_ARG, "triangle", 1),
    "index_zero_at_end": (b"v 1 2 3\nf 1 1 1 0\n", INVALID_ARG, "triangle", 1),
}
