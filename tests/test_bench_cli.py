"""CPU: bench.py's command line and its --dump-outputs writer (no GPU: the writer takes the (D, I) a search returns)."""
import numpy as np
import pytest
import torch

import bench


def test_plain_run_is_the_default_and_steps_are_checked():
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert b.full is True and b.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_writes_scores_f32_and_exact_ids_f64(tmp_path):
    D = torch.tensor([[0.75, 0.5, -float("inf")], [0.25, 0.125, 0.0]], dtype=torch.float32)
    I = torch.tensor([[(3 << 40) + 9, 5, -1], [(7 << 40) + (1 << 39) + 1, 0, 2]], dtype=torch.int64)
    bench.dump_outputs(str(tmp_path / "out"), D, I)
    S, J = np.load(tmp_path / "out" / "scores.npy"), np.load(tmp_path / "out" / "ids.npy")
    assert S.dtype == np.float32 and J.dtype == np.float64 and np.isfinite(S).all() and np.isfinite(J).all()
    want = D.numpy().copy()
    want[0, 2] = 0.0                       # the padding slot (-inf, -1): score written as 0, id -1 marks it
    assert np.array_equal(S, want) and np.array_equal(J.astype(np.int64), I.numpy())
    assert D[0, 2] == -float("inf")         # the caller's tensor is left as it was
    assert not (tmp_path / "out" / "query_rows.npy").exists()


def test_dump_above_the_limit_is_a_fixed_sample_of_rows(tmp_path):
    g = torch.Generator().manual_seed(0)
    D = torch.randn((1000, 16), generator=g)
    I = torch.randint(0, 1 << 45, (1000, 16), generator=g)
    limit = 100 * (16 * 12 + 8)
    for out in ("a", "b"):
        bench.dump_outputs(str(tmp_path / out), D, I, limit=limit)
    size = sum(f.stat().st_size - 128 for f in (tmp_path / "a").iterdir())   # minus the .npy headers
    assert size <= limit and len(list((tmp_path / "a").iterdir())) == 3
    rows = np.load(tmp_path / "a" / "query_rows.npy")
    assert len(rows) == 100 and (np.diff(rows) > 0).all()
    r = rows.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "scores.npy"), D.numpy()[r])
    assert np.array_equal(np.load(tmp_path / "a" / "ids.npy").astype(np.int64), I.numpy()[r])
    for name in ("scores.npy", "ids.npy", "query_rows.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))
    bench.dump_outputs(str(tmp_path / "a"), D[:3], I[:3], limit=limit)    # a whole dump into the same folder: no stale sample list
    assert not (tmp_path / "a" / "query_rows.npy").exists()
