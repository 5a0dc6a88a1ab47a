"""bench.py's run options: a plain run measures the mode's own line only (--full switches the
secondary measurements on), and --dump-outputs writes float64 arrays within its byte budget, the
same seeded sample of the batch rows for every array.  Host-only."""
import importlib.util
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
SECONDARY = ("no_cpu_baseline", "no_regime_p", "no_refine_input", "no_configs")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(b, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return b.parse()


def test_plain_run_has_no_secondary_measurements(monkeypatch):
    b = _bench()
    a = _parse(b, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.mode, a.full, a.dump_outputs) == (7, 2, "unit", False, None)
    assert all(getattr(a, k) for k in SECONDARY)
    assert not a.no_prof   # the event timing inside the timed steps stays


def test_full_switches_them_on_and_each_off_again(monkeypatch):
    b = _bench()
    a = _parse(b, monkeypatch, "--full")
    assert a.full and not any(getattr(a, k) for k in SECONDARY)
    a = _parse(b, monkeypatch, "--full", "--no-configs", "--no-cpu-baseline")
    assert [getattr(a, k) for k in SECONDARY] == [True, False, False, True]


def test_dump_outputs_needs_a_mode_that_returns_arrays(monkeypatch):
    b = _bench()
    assert _parse(b, monkeypatch, "--dump-outputs", "d").dump_outputs == "d"
    with pytest.raises(SystemExit):
        _parse(b, monkeypatch, "--mode", "driver", "--dump-outputs", "d")


def test_dump_outputs_small_batch_is_written_whole(tmp_path):
    import torch
    b = _bench()
    rng = np.random.default_rng(3)
    X = rng.standard_normal((5, 7)) + 1j * rng.standard_normal((5, 7))
    it = np.arange(5, dtype=np.int32)
    b.dump_outputs(tmp_path / "o", {"X": torch.from_numpy(X), "iters": it, "mu": torch.arange(5, dtype=torch.float64)})
    got = {p.name for p in (tmp_path / "o").iterdir()}
    assert got == {"X.npy", "iters.npy", "mu.npy"}
    Xd = np.load(tmp_path / "o" / "X.npy")
    assert Xd.dtype == np.float64 and Xd.shape == (5, 7, 2)
    assert np.array_equal(Xd[..., 0], X.real) and np.array_equal(Xd[..., 1], X.imag)
    itd = np.load(tmp_path / "o" / "iters.npy")
    assert itd.dtype == np.float64 and np.array_equal(itd, it)


def test_dump_outputs_samples_the_same_rows_within_the_budget(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_BUDGET", 10 * (16 * 6 + 8))   # room for 10 of the 64 rows
    rng = np.random.default_rng(4)
    X = rng.standard_normal((64, 6)) + 1j * rng.standard_normal((64, 6))
    idx = np.arange(64, dtype=np.int64)
    for d in ("a", "b"):
        b.dump_outputs(tmp_path / d, {"X": X, "idx": idx})
    rows = np.load(tmp_path / "a" / "idx.npy").astype(np.int64)
    assert rows.shape == (10,) and np.all(np.diff(rows) > 0)
    Xd = np.load(tmp_path / "a" / "X.npy")
    assert np.array_equal(Xd[..., 0] + 1j * Xd[..., 1], X[rows])
    for f in ("X.npy", "idx.npy"):   # the sample does not change from run to run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    size = sum(p.stat().st_size for p in (tmp_path / "a").iterdir())
    assert size <= 10 * (16 * 6 + 8) + 2 * 128   # the budget plus the two .npy headers
