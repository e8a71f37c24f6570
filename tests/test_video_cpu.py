"""Video mode without a GPU: the restatement of Renderer/VideoRenderer.cs (tests/video_restatement.py) against itself and against known
answers, the library's host-side tables against it bit for bit, and the new exports in the header, the ctypes mirror and the C# binding."""
import ctypes as C
import ctypes.util
import re
from pathlib import Path

import numpy as np
import pytest

import video_restatement as VR
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.renderer import video_tables

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
GEOMETRIES = [(1920, 1080, 1920, 540, 1), (640, 480, 237, 62, 2), (1280, 720, 120, 40, 4), (3, 2, 7, 5, 3)]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("case", [(5, 4, 3, 3, 2, 1), (7, 3, 4, 4, 3, 2), (2, 9, 3, 5, 2, 3), (1, 1, 3, 2, 2, 1), (9, 1, 4, 3, 3, 1), (1, 6, 3, 4, 1, 2), (12, 10, 3, 2, 1, 4),
                                  (3, 3, 4, 1, 1, 1)])
def test_scalar_and_vectorised_forms_agree(case):
    sw, sh, bpp, fw, fh, ss = case
    rng = np.random.default_rng(sum(case))
    for frame in (rng.integers(0, 256, (sh, sw, bpp), dtype=np.uint8), np.full((sh, sw, bpp), 255, np.uint8),
                  ((np.add.outer(np.arange(sh), np.arange(sw)) & 1) * 255).astype(np.uint8)[..., None].repeat(bpp, 2)):
        a = VR.blit_scalar(frame, sw, sh, bpp, fw, fh, ss)
        b = VR.blit(frame, sw, sh, bpp, fw, fh, ss)
        assert a.shape == (fh, fw, 2, 3) and np.array_equal(bits(a), bits(b)), case
        assert not np.isnan(a).any() and a.min() >= 0.0 and a.max() <= 1.0


def test_sinc_and_kernel_known_answers():
    assert VR.Sinc(f32(0.0)) == f32(1.0) and VR.Sinc(f32(9e-7)) == f32(1.0) and VR.Sinc(f32(-9e-7)) == f32(1.0)
    # at 1 and 2 the argument is MathF.PI * x in binary32, not pi: sinf of it is the rounding error of that product, not 0
    for x in (1.0, 2.0):
        pix = f32(f32(3.14159274) * f32(x))
        assert VR.Sinc(f32(x)) == f32(VR.sinf(pix) / pix) and abs(float(VR.Sinc(f32(x)))) < 1e-7
    assert float(VR.Sinc(f32(1e-6))) == pytest.approx(1.0, abs=1e-6) and VR.Sinc(f32(0.5)) == VR.Sinc(f32(-0.5))
    assert float(VR.Sinc(f32(0.5))) == pytest.approx(2.0 / np.pi, abs=1e-6)
    assert VR.LanczosKernel(f32(0.0)) == f32(1.0)
    assert VR.LanczosKernel(f32(3.0)) == f32(0.0) and VR.LanczosKernel(f32(-3.0)) == f32(0.0) and VR.LanczosKernel(f32(3.5)) == f32(0.0) and VR.LanczosKernel(f32(1e30)) == f32(0.0)
    assert VR.LanczosKernel(np.nextafter(f32(3.0), f32(0.0))) != f32(0.0)
    assert abs(float(VR.LanczosKernel(f32(1.0)))) < 1e-7 and abs(float(VR.LanczosKernel(f32(2.0)))) < 1e-7
    assert float(VR.LanczosKernel(f32(1.5))) == pytest.approx(np.sinc(1.5) * np.sinc(0.5), abs=1e-6) and VR.LanczosKernel(f32(1.5)) < 0


def test_geometry_known_answers():
    """scale / offX / offY of VideoRenderer.cs:75-81, each step rounded to binary32"""
    want = {GEOMETRIES[0]: (1920, 1080, 1.0, 0.0, 0.0),
            # 248 / 480 = 0.51666..., the smaller scale: bars left and right.  dstW = 640 * 0.51666665 = 330.66666; dstH = 247.99999237 is a tie
            # between 248 - 2^-16 and 248 and rounds to the even one, 248: offY is exactly 0
            GEOMETRIES[1]: (474, 248, float.fromhex("0x1.088888p-1"), float.fromhex("0x1.1eaaacp+6"), 0.0),
            GEOMETRIES[2]: (480, 320, 0.375, 0.0, 25.0),          # 480 / 1280 < 320 / 720: bars above and below, (320 - 270) / 2
            GEOMETRIES[3]: (21, 30, 7.0, 0.0, 8.0)}               # upscaled 7 x: 30 - 14 rows left over
    for g, (hiW, hiH, scale, offX, offY) in want.items():
        got = VR.geometry(*g)
        assert got[:2] == (hiW, hiH) and [float(v) for v in got[2:]] == [scale, offX, offY], (g, got)
        assert all(isinstance(v, np.float32) for v in got[2:])


def test_weight_sums_stay_near_one():
    """what retires the bilinear fallback (:215): over drawn source positions, positions one ulp below and above integers included, the six
    kernel values sum to [0.99, 1.01] - never <= 0"""
    rng = np.random.default_rng(7)
    pos = list(rng.uniform(-8.0, 2100.0, 30000).astype(f32)) + list(rng.uniform(-1.0, 4.0, 8000).astype(f32)) + list(rng.uniform(0.0, 70000.0, 4000).astype(f32))
    for k in list(range(-4, 40)) + [255, 256, 1023, 1919, 1920, 4095, 65536]:
        kk = f32(k)
        pos += [kk, np.nextafter(kk, f32(-np.inf)), np.nextafter(kk, f32(np.inf)), f32(kk + f32(0.5)), f32(kk + f32(1e-6)), f32(kk - f32(1e-6))]
    lo, hi = 2.0, 0.0
    for s in pos:
        p0, k, total = VR.axis_weights(f32(s))
        assert p0 == int(np.floor(s)) and len(k) == 6
        lo, hi = min(lo, float(total)), max(hi, float(total))
    assert len(pos) >= 42000 and 0.99 <= lo and hi <= 1.01, (lo, hi)


@pytest.mark.parametrize("g", GEOMETRIES + [(1, 1, 1, 1, 1), (1, 50, 9, 4, 2), (50, 1, 3, 7, 1), (4000, 3000, 80, 45, 1)])
def test_library_tables_equal_the_restatement(product_lib, g):
    x0, wx, y0, wy, geom = VR.tables(*g)
    lx0, lwx, ly0, lwy, lgeom = video_tables(*g, lib=product_lib)
    assert np.array_equal(x0, lx0) and np.array_equal(y0, ly0)
    assert np.array_equal(bits(wx), bits(lwx)) and np.array_equal(bits(wy), bits(lwy))
    assert [float(v).hex() for v in geom] == [float(v).hex() for v in lgeom]


def test_table_hook_refuses_bad_arguments(product_lib):
    fn = product_lib.ycge_host_video_tables
    fn.restype, fn.argtypes = abi.VIDEO_HOOK_PROTOTYPES["ycge_host_video_tables"]
    a = np.zeros(64, np.float32)
    p = a.ctypes.data
    assert fn(2, 2, 1, 1, 1, p, p, p, p, p) == abi.YCGE_OK
    for args in ((0, 2, 1, 1, 1), (2, 0, 1, 1, 1), (2, 2, 0, 1, 1), (2, 2, 1, 0, 1), (2, 2, 1, 1, 0), (2, 2, 1, 1, 5000), (2, 2, 2 ** 30, 1, 1)):
        assert fn(*args, p, p, p, p, p) == abi.YCGE_ERR_INVALID_ARG, args
    assert fn(2, 2, 1, 1, 1, None, p, p, p, p) == abi.YCGE_ERR_INVALID_ARG


def test_byte_to_unit_formula_of_the_kernel_is_the_division():
    """k_video_blit forms byte / 255.0f as q = b * fl(1/255), r = fma(-255, q, b), fma(r, fl(1/255), q): equal to the correctly rounded
    division for all 256 bytes (fmaf from libm: exact)"""
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float] * 3
    k = f32(f32(1.0) / f32(255.0))
    for b in range(256):
        x = f32(b)
        q = f32(x * k)
        r = f32(libm.fmaf(-255.0, float(q), float(x)))
        assert f32(libm.fmaf(float(r), float(k), float(q))) == f32(x / f32(255.0)), b


def test_exports_are_declared_in_every_mirror(product_lib):
    header = (ROOT / "include" / "ycge.h").read_text()
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text()
    cs = (ROOT / "bindings" / "csharp" / "Ycge.cs").read_text()
    for name in ("ycge_video_blit", "ycge_video_blit_ansi"):
        assert re.search(r"\bint " + name + r"\(ycge_ctx \*ctx, const uint8_t \*frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel,", header), name
        assert name in abi.EXPORTED_SYMBOLS and hasattr(product_lib, name)
        assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern int " + name + r"\(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel,", cs), name
    assert len(abi._PROTOTYPES["ycge_video_blit"][1]) == 9 and len(abi._PROTOTYPES["ycge_video_blit_ansi"][1]) == 16
    for name in abi.VIDEO_HOOK_PROTOTYPES:
        assert re.search(r"\bint " + name + r"\(", hooks) and name not in header and hasattr(product_lib, name), name
    assert "#define YCGE_ABI_VERSION 10" in header and abi.YCGE_ABI_VERSION == 10


def test_video_exports_are_guarded_and_the_sources_registered():
    """ycge_video.cpp / ycge_video.hip are built; the four exports are function-try-blocks into abi_catch where the barrier test of
    tests/test_host_cpu.py reads them (beside the calls they mirror), and ycge_video.cpp opens no extern "C" block of its own"""
    from yetanotherconsolegameengine_amd import build
    assert "ycge_video.cpp" in build.SOURCES and "ycge_video.hip" in build.SOURCES
    csrc = Path(abi.__file__).resolve().parent / "csrc"
    assert 'extern "C"' not in (csrc / "ycge_video.cpp").read_text()
    for fname, names in (("ycge_chexel.cpp", ("ycge_video_blit", "ycge_host_video_tables", "ycge_test_video_blit")), ("ycge_ansi.cpp", ("ycge_video_blit_ansi",))):
        text = (csrc / fname).read_text()
        for n in names:
            m = re.search(r"^int " + n + r"\([^{;]*?\)\ntry \{\n(.*?)\n\}\ncatch \(\.\.\.\) \{ return ycge_host::abi_catch\(", text, re.S | re.M)
            assert m, (fname, n)


def test_video_wrapper_only_calls_what_is_declared():
    """bindings/csharp/HipVideoWrapper.cs: every Ycge.ycge_* call names a declared import with the declared number of arguments; the seam's
    members are there and the blit passes the reader's frame"""
    cs = (ROOT / "bindings" / "csharp" / "Ycge.cs").read_text()
    imports = {m.group(1): len([p for p in m.group(2).split(",") if p.strip()])
               for m in re.finditer(r"\[DllImport\(Lib\)\]\s*public static extern \w+ (ycge_\w+)\(([^)]*)\);", cs)}
    text = re.sub(r"//[^\n]*", "", (ROOT / "bindings" / "csharp" / "HipVideoWrapper.cs").read_text())
    seen = set()
    for m in re.finditer(r"Ycge\.(ycge_\w+)\(", text):
        name = m.group(1)
        assert name in imports, name
        i, depth, args, cur = m.end(), 1, [], ""
        while depth:
            ch = text[i]
            if ch in "([{":
                depth += 1
            elif ch in ")]}":
                depth -= 1
                if depth == 0:
                    break
            if ch == "," and depth == 1:
                args.append(cur); cur = ""
            else:
                cur += ch
            i += 1
        if cur.strip():
            args.append(cur)
        assert len(args) == imports[name], (name, args)
        seen.add(name)
    assert {"ycge_video_blit", "ycge_video_blit_ansi", "ycge_resize", "ycge_create", "ycge_destroy", "ycge_alloc_host_buffer", "ycge_free_host_buffer",
            "ycge_ansi_stream_bound"} <= seen
    assert "public partial class RaytraceEntity" in text and ": IConsoleRenderer" in text and "IFrameReader reader" in text
    for member in ("void SetCamera(Vec3", "void SetFov(float", "void TryFlipAndBlit(Framebuffer", "void Resize(Framebuffer"):
        assert member in text, member
    assert "reader.GetCurrentFramePtr()" in text and "reader.Width" in text and "reader.Height" in text and "useRGBA ? 4 : 3" in text
    assert "ycge_scene_upload" not in text and "GCHandle" not in text
