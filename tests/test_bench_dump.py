"""bench.py --dump-outputs without a GPU: the argument contract and the writer's budget, dtypes and
fixed sample (the GPU run itself: tests/test_gpu_bench_contract.py)."""
import numpy as np
import pytest

import bench


def _outs(torch, B, dtype):
    g = torch.Generator().manual_seed(7)
    return dict(X=torch.rand(B, 6, 21, generator=g, dtype=dtype),
                U=torch.rand(B, 2, 20, generator=g, dtype=dtype),
                K_feedback=torch.rand(B, 2, 6, 20, generator=g, dtype=dtype),
                iters=torch.full((B,), 10, dtype=torch.int32),
                best_idx=torch.tensor([3], dtype=torch.int64),
                best_cost=torch.tensor([0.5], dtype=dtype),
                winner_X=torch.rand(6, 21, generator=g, dtype=dtype))


def test_steps_and_dump_arguments():
    a = bench.parse_args(["--steps", "7", "--warmup", "0", "--dump-outputs", "out"])
    assert (a.steps, a.warmup, a.dump_outputs) == (7, 0, "out")
    assert bench.parse_args([]).dump_outputs is None
    for argv in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(argv)


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    a = bench.parse_args(["--full", "--no-extra", "--cpu-seconds", "2"])
    assert a.full and a.no_extra and not a.no_cpu_baseline and a.cpu_seconds == 2.0


def test_small_batch_is_written_whole(tmp_path):
    torch = pytest.importorskip("torch")
    outs = _outs(torch, 1024, torch.float64)
    info = bench.dump_step_outputs(tmp_path, outs, 1024, torch)
    assert not info["sampled"] and info["problems"] == 1024
    assert not (tmp_path / "sample_index.npy").exists()
    for name, t in outs.items():
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float64
        np.testing.assert_array_equal(a, t.double().numpy())


def test_large_batch_keeps_a_fixed_sample_within_the_budget(tmp_path):
    torch = pytest.importorskip("torch")
    B = 65536
    outs = _outs(torch, B, torch.float32)
    first = bench.dump_step_outputs(tmp_path / "a", outs, B, torch)
    second = bench.dump_step_outputs(tmp_path / "b", outs, B, torch)
    assert first["sampled"] and 0 < first["problems"] < B and first == second
    files = sorted((tmp_path / "a").glob("*.npy"))
    assert sum(f.stat().st_size for f in files) <= bench.DUMP_BUDGET_BYTES
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    np.testing.assert_array_equal(idx, np.load(tmp_path / "b" / "sample_index.npy"))
    assert idx.dtype == np.float64 and (np.diff(idx) > 0).all() and len(idx) == first["problems"]
    idx = idx.astype(np.int64)
    for name in ("X", "U", "K_feedback"):
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, outs[name].numpy()[idx])
    assert np.load(tmp_path / "a" / "iters.npy").dtype == np.float64
    # arrays that are not per problem are written whole
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "winner_X.npy"), outs["winner_X"].numpy())
    assert np.load(tmp_path / "a" / "best_idx.npy").tolist() == [3.0]
