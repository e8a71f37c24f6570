"""The inputs of tests/test_gpu_video_quadrants.py (test infrastructure), in a module of their own so that tests/test_video_quadrants_cpu.py
can assert, without a GPU, that they reach what the GPU tests are there for: every mask, flat and unflat cells under min_contrast, taps
clamped at each frame edge, the frame's last pixel as a 3-byte tap, and quadrant sums whose halves do not add up to the serial sum."""
import numpy as np

# the kernel alone: (src_w, src_h, bytes per pixel, fbW, fbH, ss).  fbW 1 / 63 / 64 / 65 / 130: a lone lane, a partial wavefront, an exact one,
# a second and a third group; fbH 1 and 3; ss 2, 4 and 6 (ss / 2 odd); sources that upscale (7 x 5; 1 x 1: every tap clamped), downscale
# (40 x 30 into 20 x 5, 320 x 200 into 5 x 2) and letterbox both ways (64 x 6, 6 x 64); the context tests' shape last
HOOK_CASES = [(7, 5, 3, 1, 1, 2), (7, 5, 4, 63, 1, 2), (7, 5, 3, 64, 3, 2), (7, 5, 3, 65, 3, 4), (7, 5, 4, 130, 3, 2), (7, 5, 3, 130, 1, 6), (1, 1, 3, 65, 1, 2),
              (1, 1, 4, 5, 3, 6), (40, 30, 4, 20, 5, 4), (40, 30, 3, 20, 5, 2), (320, 200, 3, 5, 2, 2), (320, 200, 4, 5, 2, 6), (64, 6, 3, 63, 3, 2), (6, 64, 4, 64, 3, 4),
              (6, 64, 3, 7, 3, 6), (9, 7, 4, 11, 2, 4), (16, 12, 3, 65, 9, 2)]
# the scalar form is a Python loop over every tap: these cases of the list are small enough for it, and between them hold every ss, both
# pixel sizes, both scaling directions and both letterboxes
SCALAR_CASES = [c for c in HOOK_CASES if c[3] * c[4] * c[5] * c[5] * 2 <= 1600]

# A frame of all 255 comes back as exactly 1.0 where every sample's 36 products add up to 1 or more: the normalised weights of an axis sum to 1
# within an ulp, not to 1, so on most geometries the reference itself shows 0.9999999 in places (ycge_video_blit too).  On these cases of the
# list the restatement gives 1.0 in every value (tests/test_video_quadrants_cpu.py asserts it); on all the others the all-255 frame is held
# to the restatement bit for bit like any other frame
ONES_EXACT_CASES = [(7, 5, 3, 1, 1, 2), (320, 200, 3, 5, 2, 2), (320, 200, 4, 5, 2, 6)]

# the context tests: a 16 x 12 BGR source into 65 x 9 chexels at ss 2 (two workgroups a row), and a 40 x 30 BGRA one into 20 x 5 at ss 4
CONTEXT_CASES = [(16, 12, 3, 65, 9, 2), (40, 30, 4, 20, 5, 4)]


def case_id(c):
    return "%dx%dx%d-%dx%d-ss%d" % c


def noise(src_w, src_h, bpp, seed=0):
    """a seeded uniform-noise frame (height, width, bytes per pixel)"""
    return np.random.default_rng([src_w, src_h, bpp, seed]).integers(0, 256, (src_h, src_w, bpp), dtype=np.uint8)


def constant(src_w, src_h, bpp, value):
    return np.full((src_h, src_w, bpp), value, np.uint8)


def drawn(src_w, src_h, bpp, seed=6):
    """noise with one flat block in a corner, wide enough that some chexels see nothing else through their 6 x 6 taps: the one-colour mask
    occurs at min_contrast 0 only where all four sub-cell bytes are equal.  The seed is one whose noise also holds the rare diagonal mask in both
    context geometries (tests/test_video_quadrants_cpu.py asserts that every mask occurs)"""
    f = noise(src_w, src_h, bpp, seed)
    f[:src_h // 2 + 2, :src_w // 2, :3] = (40, 90, 200)
    return f


def sequence(src_w, src_h, bpp):
    """the four frames of the context tests: a frame, the same again, one with a changed region, that one again (shown under a moved layer)"""
    a = drawn(src_w, src_h, bpp)
    b = a.copy()
    b[src_h - 4:src_h - 1, src_w - 5:src_w - 1, :3] = noise(4, 3, 3, 2)
    return [a, a.copy(), b, b.copy()]
