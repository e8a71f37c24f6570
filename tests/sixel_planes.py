"""Register planes for the sixel tests (tests/test_sixel_cpu.py, tests/test_gpu_sixel.py): drawn ones for a size, and the built ones that
sit on the encoder's seams - the 64-column trips of its walk, the omitted tail of a line, the most lines a band can have."""
import numpy as np

CANARY = 0xA5
HEIGHTS = (1, 5, 6, 7, 12, 13)
VIEWPORTS = ((0, 0), (9, 99), (999, 9))


def drawn(w, h):
    """three planes of w x h: every pixel its own draw of the 216 registers; a few registers in runs of drawn lengths (long ones among
    them) that pay no heed to the rows; one register with others sprinkled in"""
    rng = np.random.default_rng([w, h])
    noise = rng.integers(0, 216, (h, w)).astype(np.uint8)
    few = rng.choice(216, 5, replace=False)
    lengths = rng.choice([1, 2, 3, 4, 5, 9, 10, 11, 63, 64, 65, 99, 100, 101, 700], w * h + 1)
    runs = np.repeat(few[rng.integers(0, 5, lengths.size)], lengths)[:w * h].reshape(h, w).astype(np.uint8)
    if h > 1:
        runs[1::2] = np.roll(runs[::2], 1, axis=1)[:runs[1::2].shape[0]]          # (rows that agree but for a shift: sixels with several bits)
    sparse = np.full((h, w), int(few[0]), np.uint8)
    mask = rng.random((h, w)) < 0.03
    sparse[mask] = rng.integers(0, 216, int(mask.sum()))
    return noise, runs, sparse


def _one_colour():
    return np.full((13, 130), 100, np.uint8)


def _all_registers_in_one_band():
    return np.random.default_rng(216).permutation(216).reshape(6, 36).astype(np.uint8)


def _only_pixel_in_the_last_column():
    p = np.full((7, 129), 3, np.uint8)
    p[4, 128] = 200
    p[6, 128] = 201
    return p


def _only_pixel_in_column_0():
    p = np.full((7, 129), 3, np.uint8)
    p[2, 0] = 200
    p[6, 0] = 201
    return p


def _runs_of_3_and_4_before_a_multiple_of_64():
    p = np.zeros((36, 200), np.uint8)
    band = 0
    for n in (3, 4):
        for before in (1, 2, 3):
            p[6 * band:6 * band + 6, 64 - before:64 - before + n] = 5
            p[6 * band + 1:6 * band + 3, 128 - before:128 - before + n] = 77
            p[6 * band + 5, 192 - before:192 - before + n] = 215
            band += 1
    return p


def _run_of_1000_to_the_last_column():
    p = np.zeros((6, 1100), np.uint8)
    p[:, 100:] = 9
    p[3, 100:] = 10
    return p


def _300_bands_of_8_columns():
    return np.random.default_rng(300).integers(0, 216, (1800, 8)).astype(np.uint8)


SEAMS = {
    "one_colour": _one_colour,
    "all_216_in_one_band": _all_registers_in_one_band,
    "only_pixel_in_the_last_column": _only_pixel_in_the_last_column,
    "only_pixel_in_column_0": _only_pixel_in_column_0,
    "runs_of_3_and_4_before_a_multiple_of_64": _runs_of_3_and_4_before_a_multiple_of_64,
    "run_of_1000_to_the_last_column": _run_of_1000_to_the_last_column,
    "300_bands_of_8_columns": _300_bands_of_8_columns,
}
