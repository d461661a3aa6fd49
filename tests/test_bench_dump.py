"""not-gpu: bench.py --dump-outputs — what is written (float32, the indices in float64), the byte budget, and that the seeded sample of a
large output is the same in every run."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_dump_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_small_output_is_written_whole(tmp_path):
    bench = _bench()
    y = torch.randint(0, 256, (5, 4, 6, 3), dtype=torch.uint8)             # the uint8 BGR form of the output
    assert bench.dump_outputs(str(tmp_path), "sr", y) == [0, 1, 2, 3, 4]
    a = np.load(tmp_path / "sr.npy")
    assert a.dtype == np.float32 and np.array_equal(a, y.float().numpy())
    assert np.load(tmp_path / "sr_index.npy").tolist() == [0, 1, 2, 3, 4]


def test_large_output_is_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    bench = _bench()
    row = 3 * 8 * 16 * 4                                                     # bytes of one image in float32
    monkeypatch.setattr(bench, "DUMP_BYTES", (1 << 16) + 7 * row)            # room for 7 of 40 images
    y = torch.randn(40, 3, 8, 16, dtype=torch.float16)
    keep = bench.dump_outputs(str(tmp_path / "a"), "sr", y)
    assert len(keep) == 7 and keep == sorted(set(keep)) and keep != list(range(7))
    assert bench.dump_outputs(str(tmp_path / "b"), "sr", y.clone()) == keep            # same choice in every run
    a = np.load(tmp_path / "a" / "sr.npy")
    assert a.dtype == np.float32 and np.array_equal(a, y[keep].float().numpy())
    idx = np.load(tmp_path / "a" / "sr_index.npy")
    assert idx.dtype == np.float64 and idx.tolist() == keep
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= bench.DUMP_BYTES


def test_images_of_different_widths_are_one_file_each(tmp_path, monkeypatch):
    bench = _bench()
    ys = [torch.randn(3, 8, 4 * w) for w in (32, 48, 16, 64, 32)]
    monkeypatch.setattr(bench, "DUMP_BYTES", (1 << 16) + sum(t.numel() * 4 for t in ys[:3]))
    keep = bench.dump_outputs(str(tmp_path), "sr_strip", ys)
    assert 1 <= len(keep) < 5
    assert sorted(os.listdir(tmp_path)) == sorted(["sr_strip_%04d.npy" % i for i in keep] + ["sr_strip_index.npy"])
    for i in keep:
        assert np.array_equal(np.load(tmp_path / ("sr_strip_%04d.npy" % i)), ys[i].numpy())
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= bench.DUMP_BYTES
