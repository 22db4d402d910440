"""bench.py --dump-outputs (no GPU): the files the dump writes, their dtypes, the byte budget and the seeded sample."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _img(units, rows, width, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (units, rows, width, 3), dtype=np.uint8)


def test_small_output_is_dumped_whole(bench, tmp_path):
    img = _img(2, 9, 16)
    bench.dump_outputs(str(tmp_path / "d"), img, [(0, 0), (1, 2)], rank=0, world=1)
    got = np.load(tmp_path / "d" / "image.npy")
    assert got.dtype == np.float32 and got.shape == img.shape and np.array_equal(got, img.astype(np.float32))
    units = np.load(tmp_path / "d" / "units.npy")
    assert units.dtype == np.float64 and units.tolist() == [[0, 0], [1, 2]]


def test_large_output_is_a_fixed_sample_within_budget(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 * 1000)
    img = _img(3, 40, 128)                                    # 46 080 bytes of RGB8 -> 184 KB as float32: over budget
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), img, [(0, 0), (0, 1), (0, 2)], rank=0, world=1)
    total = sum(f.stat().st_size for f in (tmp_path / "a").iterdir())
    assert total <= 64 * 1000
    assert not (tmp_path / "a" / "image.npy").exists()
    val, idx = np.load(tmp_path / "a" / "image_sample.npy"), np.load(tmp_path / "a" / "image_sample_index.npy")
    assert val.dtype == np.float32 and idx.dtype == np.float64 and val.shape == (len(idx), 3) and len(idx) > 1000
    assert np.all(np.diff(idx) > 0) and idx[-1] < img.size // 3
    assert np.array_equal(val, img.reshape(-1, 3)[idx.astype(np.int64)].astype(np.float32))
    assert np.array_equal(idx, np.load(tmp_path / "b" / "image_sample_index.npy"))      # same pixels every run


def test_ranks_write_their_own_files(bench, tmp_path):
    for r in range(2):
        bench.dump_outputs(str(tmp_path), _img(1, 4, 8, seed=r), [(r, 0)], rank=r, world=2)
    assert sorted(f.name for f in tmp_path.iterdir()) == ["image_rank0.npy", "image_rank1.npy", "units_rank0.npy", "units_rank1.npy"]


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--frame", "--dump-outputs", "x"]])
def test_bad_arguments_are_refused(bench, monkeypatch, argv):
    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit):
        bench.parse_args()
