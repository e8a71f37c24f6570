"""MeshLoader.FromObj (RayTracing/MeshLoader.cs:12-149) restated in plain Python: the yardstick of ycge_obj_parse_host and of the device
parse.  It shares no code with yetanotherconsolegameengine_amd/mesh_loader.py or with the library.

The rules (include/ycge.h states them for the library):
  lines     StreamReader.ReadLine ends a line at \\n, \\r\\n or a lone \\r; the last line needs no terminator; a UTF-8 byte-order mark at
            offset 0 is skipped; lines count from 1.  An empty line or one whose first byte is '#' is skipped (" # x" is not).
  tokens    Split((char[])null, RemoveEmptyEntries) = char.IsWhiteSpace: inside a line, in ASCII, space \\t \\v \\f.  0x1C..0x1F are NOT
            separators for .NET (they are for Python's str.split).
  v         first token exactly "v", >= 4 tokens: tokens 1..3 parsed, the rest never looked at.  Fewer tokens: nothing.
  f         first token exactly "f", >= 4 tokens: every token cut at its first '/', ParseIndex: empty -> 0, i > 0 -> i - 1, else count + i
            (count: positions so far, at this line); fan (v0, v[k-1], v[k]).  0 <= index < FINAL count is checked after the file.
  floats    [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)?, CORRECTLY rounded to binary32 (nearest, ties to even): done here with
            fractions.Fraction, exactly.  -0 stays -0; overflow +-inf; underflow subnormal or zero.
  integers  [+-]? digits within int32.
  refusals  (status, kind, number), in this order: the first line in file order with a malformed float / integer token (INVALID_ARG) or a
            byte >= 0x80 outside a comment (UNSUPPORTED; the byte decides for its line); [more than 2^28 triangles]; no position or no
            triangle; an index out of range, named by the lowest triangle counted from 0.
  tail      binary32, operation by operation: box over the used vertices (-0 orders below +0; the reference's sign of a zero extreme
            follows HashSet enumeration order), c = (min + max) * 0.5f, maxExtent by three compares (<= 0 -> 1), s = target / maxExtent,
            every vertex (p - c) * s unless a bound is infinite; p * scale + t only when scale != 1 or t != 0; gather; bounds over corners.
"""
from __future__ import annotations

import re
from fractions import Fraction
from functools import lru_cache

import numpy as np

INVALID_ARG, UNSUPPORTED = -1, -4
_FLOAT = re.compile(rb"([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?")
_INT = re.compile(rb"[+-]?[0-9]+")
_TOKEN = re.compile(rb"[^ \t\x0b\x0c]+")


class Refusal(Exception):
    def __init__(self, status, kind, number=None):
        super().__init__(f"{status} {kind} {number}")
        self.status, self.kind, self.number = status, kind, number


def round_binary32(v: Fraction) -> int:
    """the bits of the binary32 nearest to v >= 0, ties to even (overflow: inf)"""
    if v == 0:
        return 0
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    assert Fraction(2) ** e <= v < Fraction(2) ** (e + 1)
    e = max(e, -126)
    quantum = Fraction(2) ** (e - 23)
    m = v / quantum
    k = m.numerator // m.denominator
    rem = m - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k & 1):
        k += 1
    if k == 1 << 24:
        k, e = 1 << 23, e + 1
    if k < 1 << 23:                      # subnormal (e == -126)
        return k
    if e + 127 >= 255:
        return 0x7F800000
    return ((e + 127) << 23) | (k - (1 << 23))


@lru_cache(maxsize=1 << 16)
def float_bits(tok: bytes):
    """the binary32 bits of a float token, None if malformed"""
    m = _FLOAT.fullmatch(tok)
    if not m:
        return None
    sign, ip, fp, fp2, ex = m.groups()
    digits = (ip or b"") + (fp or b"") + (fp2 or b"")
    frac = len(fp or b"") + len(fp2 or b"")
    sbit = 0x80000000 if sign == b"-" else 0
    w = int(digits)
    if w == 0:
        return sbit
    q = (int(ex) if ex else 0) - frac
    lead = len(str(w)) + q               # 10^(lead-1) <= v < 10^lead
    if lead - 1 >= 39:
        return sbit | 0x7F800000
    if lead <= -46:                      # v < 1e-46 < 2^-150: below half the smallest subnormal
        return sbit
    v = Fraction(w) * Fraction(10) ** q
    return sbit | round_binary32(v)


def int_value(tok: bytes):
    if not _INT.fullmatch(tok):
        return None
    v = int(tok)
    return v if -(1 << 31) <= v < (1 << 31) else None


def split_lines(data: bytes):
    body = data[3:] if data[:3] == b"\xef\xbb\xbf" else data
    lines = re.split(rb"\r\n|\n|\r", body)
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def parse(data: bytes):
    """(positions uint32 [nv, 3] - the floats' bits, faces int32 [nt, 3], n_lines) or raises Refusal"""
    if not data:
        raise Refusal(INVALID_ARG, "empty")
    lines = split_lines(data)
    pos, faces = [], []
    for ln, line in enumerate(lines, 1):
        if len(line) == 0 or line[:1] == b"#":
            continue
        if any(b >= 0x80 for b in line):
            raise Refusal(UNSUPPORTED, "line", ln)
        tok = _TOKEN.findall(line)
        if not tok:
            continue
        if tok[0] == b"v" and len(tok) >= 4:
            xyz = [float_bits(t) for t in tok[1:4]]
            if None in xyz:
                raise Refusal(INVALID_ARG, "line", ln)
            pos.append(xyz)
        elif tok[0] == b"f" and len(tok) >= 4:
            idx = []
            for t in tok[1:]:
                part = t.split(b"/")[0]
                if part == b"":
                    idx.append(0)
                    continue
                i = int_value(part)
                if i is None:
                    raise Refusal(INVALID_ARG, "line", ln)
                idx.append(i - 1 if i > 0 else len(pos) + i)
            for k in range(2, len(idx)):
                faces.append((idx[0], idx[k - 1], idx[k]))
    if len(faces) > 1 << 28:
        raise Refusal(INVALID_ARG, "too many")
    if not pos or not faces:
        raise Refusal(INVALID_ARG, "none")
    for k, f in enumerate(faces):
        if any(i < 0 or i >= len(pos) for i in f):
            raise Refusal(INVALID_ARG, "triangle", k)
    return np.array(pos, dtype=np.uint32).reshape(-1, 3), np.array(faces, dtype=np.int32).reshape(-1, 3), len(lines)


def _ordered(bits: np.ndarray) -> np.ndarray:
    """uint32 keys in the floats' order, -0 below +0"""
    bits = bits.astype(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def _extremes(values: np.ndarray):
    """min and max over the rows of float32 [n, 3], NaN never an extreme; nothing: +inf / -inf"""
    mn, mx = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
    for a in range(3):
        col = values[:, a]
        col = col[~np.isnan(col)]
        if col.size:
            key = _ordered(col.view(np.uint32))
            mn[a], mx[a] = col[np.argmin(key)], col[np.argmax(key)]
    return mn, mx


def triangles(pos_bits: np.ndarray, faces: np.ndarray, normalize=True, target_size=1.0, scale=1.0, translate=(0.0, 0.0, 0.0)):
    """MeshLoader.cs:57-96, 107-148 -> (triangles float32 [nt, 3, 3], bounds float32 [6] = min xyz, max xyz)"""
    f32 = np.float32
    pos = pos_bits.astype(np.uint32).view(np.float32).copy()
    with np.errstate(all="ignore"):
        if normalize:
            used = np.unique(faces.reshape(-1))
            mn, mx = _extremes(pos[used])
            if not (np.isinf(mn).any() or np.isinf(mx).any()):
                c = (mn + mx) * f32(0.5)
                r = mx - mn
                ext = r[0]
                if r[1] > ext:
                    ext = r[1]
                if r[2] > ext:
                    ext = r[2]
                if ext <= 0:
                    ext = f32(1.0)
                s = f32(target_size) / ext
                pos = ((pos - c).astype(np.float32) * s).astype(np.float32)
        t = np.asarray(translate, dtype=np.float32)
        if f32(scale) != f32(1.0) or t[0] != 0 or t[1] != 0 or t[2] != 0:
            pos = ((pos * f32(scale)).astype(np.float32) + t).astype(np.float32)
    tris = np.ascontiguousarray(pos[faces])
    mn, mx = _extremes(tris.reshape(-1, 3))
    return tris, np.concatenate([mn, mx]).astype(np.float32)
