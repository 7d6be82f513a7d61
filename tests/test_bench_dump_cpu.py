"""`bench.py --dump-outputs DIR`: the frames of the last timed clip as float .npy files, 64 MB at most, at the same
positions on every run (so that two builds can be compared output for output).  No GPU needed: dump_outputs is fed host
tensors of the shapes the timed path returns."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(files):
    return {os.path.basename(p)[:-4]: np.load(p) for p in files}


def test_small_output_is_written_whole(tmp_path):
    f = torch.rand(2, 3, 4, 5, generator=torch.Generator().manual_seed(1))
    got = _load(bench.dump_outputs(f, str(tmp_path)))
    assert sorted(got) == ["frames_row_mean", "frames_sample"]
    assert got["frames_sample"].dtype == np.float32 and np.array_equal(got["frames_sample"], f.reshape(-1).numpy())
    assert got["frames_row_mean"].dtype == np.float64 and got["frames_row_mean"].shape == (2, 3, 4)
    assert np.allclose(got["frames_row_mean"], f.double().mean(-1).numpy(), rtol=0, atol=1e-12)


def test_full_clip_is_sampled_within_64_mb_at_fixed_positions(tmp_path):
    """one clip of the headline workload: 25 x 3 x 576 x 1024 fp32 = 177 MB, more than the budget"""
    f = torch.rand(bench.T, 3, bench.H, bench.W, generator=torch.Generator().manual_seed(2))
    a = bench.dump_outputs(f, str(tmp_path / "a"))
    b = bench.dump_outputs(f.clone(), str(tmp_path / "b"))
    assert sum(os.path.getsize(p) for p in a) <= 64 << 20
    da, db = _load(a), _load(b)
    assert da["frames_sample"].shape == (bench.DUMP_SAMPLE,) and da["frames_sample"].dtype == np.float32
    assert da["frames_row_mean"].shape == (bench.T, 3, bench.H)
    for k in da:
        assert np.array_equal(da[k], db[k]), k
    # the sample is the values at sorted, distinct positions drawn with seed 0: check them against the tensor itself
    pos = torch.randperm(f.numel(), generator=torch.Generator().manual_seed(0))[:bench.DUMP_SAMPLE].sort().values
    assert np.array_equal(da["frames_sample"], f.reshape(-1)[pos].numpy())
    # a change anywhere in the clip shows in the row means even where the sample does not look
    g = f.clone()
    g[7, 1, 100, 3] += 0.5
    dg = _load(bench.dump_outputs(g, str(tmp_path / "g")))
    assert not np.array_equal(dg["frames_row_mean"], da["frames_row_mean"])


def test_dump_in_shard_mode_is_an_error_before_any_launch(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--dump-outputs", "out"])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "--dump-outputs" in str(e.value.code)
