"""CPU test of bench.py --dump-outputs (dump_outputs): a frame within the budget is written whole; a larger one as the same
seeded sample of pixels every time, with row and column sums over every pixel; at most 64 MB in all."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_small_frame_is_written_whole(tmp_path):
    bench = load_bench()
    img = np.random.default_rng(0).random((36, 64, 3), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "out"), img)
    assert os.listdir(tmp_path / "out") == ["image.npy"]
    assert np.array_equal(np.load(tmp_path / "out" / "image.npy"), img)


def test_4k_frame_is_a_fixed_sample_within_64_mb(tmp_path):
    bench = load_bench()
    H, W = 2160, 3840
    img = np.arange(H * W * 3, dtype=np.float32).reshape(H, W, 3)
    for k in (0, 1):
        bench.dump_outputs(str(tmp_path / str(k)), img)
    files = sorted(os.listdir(tmp_path / "0"))
    assert files == ["image_col_sums.npy", "image_row_sums.npy", "image_sample.npy", "image_sample_index.npy"]
    assert sum(os.path.getsize(tmp_path / "0" / f) for f in files) <= 64 << 20
    a = {f: np.load(tmp_path / "0" / f) for f in files}
    for f in files:
        assert a[f].dtype in (np.float32, np.float64)
        assert np.array_equal(a[f], np.load(tmp_path / "1" / f)), f     # the same sample from run to run
    idx = a["image_sample_index.npy"].astype(np.int64)
    assert len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < H * W
    assert np.array_equal(a["image_sample.npy"], img.reshape(-1, 3)[idx])
    assert np.allclose(a["image_row_sums.npy"], img.astype(np.float64).sum(axis=1))
    assert np.allclose(a["image_col_sums.npy"], img.astype(np.float64).sum(axis=0))
