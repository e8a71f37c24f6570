"""bench.py --dump-outputs: what the timed path computed in its last step, as float32 .npy files within a fixed budget - on CPU."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def frame(h, w, seed):
    rng = np.random.default_rng(seed)
    return {"taa_history": rng.random((h, w, 3), dtype=np.float32), "current_hdr": rng.random((h, w, 3), dtype=np.float32)}


def test_buffers_within_the_budget_are_written_whole(tmp_path):
    a = frame(27, 96, 1)
    bench.dump_outputs(tmp_path / "out", a)
    for k, v in a.items():
        got = np.load(tmp_path / "out" / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, v)


def test_buffers_over_the_budget_are_cut_to_one_fixed_sample_of_pixels(tmp_path):
    a = frame(90, 160, 2)                 # 2 x 172 800 B
    budget = 48_000                       # 2000 pixels of 24 B
    bench.dump_outputs(tmp_path / "x", a, budget=budget)
    bench.dump_outputs(tmp_path / "y", a, budget=budget)
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(90 * 160, 2000, replace=False))
    total = 0
    for k, v in a.items():
        x, y = np.load(tmp_path / "x" / f"{k}.npy"), np.load(tmp_path / "y" / f"{k}.npy")
        assert x.shape == (2000, 3) and x.dtype == np.float32 and np.array_equal(x, y)
        assert np.array_equal(x, v.reshape(-1, 3)[idx])          # the same pixels in every buffer, in pixel order
        total += x.nbytes
    assert total <= budget


def test_the_default_budget_holds_a_full_headline_frame_and_samples_a_4k_one(tmp_path):
    z = np.zeros((1080, 1920, 3), dtype=np.float32)               # config 4's 1920x1080 trace grid: two buffers, 50 MB, whole
    bench.dump_outputs(tmp_path / "c4", {"taa_history": z, "current_hdr": z})
    assert np.load(tmp_path / "c4" / "taa_history.npy").shape == z.shape
    z = np.zeros((2160, 3840, 3), dtype=np.float32)               # config 5's 3840x2160 trace grid: sampled to the budget
    bench.dump_outputs(tmp_path / "c5", {"taa_history": z, "current_hdr": z})
    assert sum(p.stat().st_size for p in (tmp_path / "c5").iterdir()) <= bench.DUMP_BUDGET_BYTES + 2 * 4096
