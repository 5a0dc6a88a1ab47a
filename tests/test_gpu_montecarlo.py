"""GPU tests of the Monte-Carlo sweep ace_amd.montecarlo.vs_m (the reference's Vs_M.m:163-226 loop: device
synth -> recovery pipeline -> Evaluation_H on the device, only the metrics leaving it).

The metrics are checked against the numpy restatement (tests/eval_ref.py) on the pipeline's own X, with the
parity bars of tests/test_gpu_evaluate.py.  No recovery-quality threshold is asserted: none has been measured.
"""
import math
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import eval_ref as ER  # noqa: E402

pytestmark = pytest.mark.gpu

TX = RX = 8
COUNT, SEED, MAXITER = 16, 7, 60


def _recover(gpu, method, M, count):
    """The sweep point's recovery of realisations 0 .. count - 1, restated: the same synth, partitions and pipeline
    call on the sweep's first chunk (vs_m solves whole chunks of montecarlo.CHUNK realisations, because the
    pipeline's rounding depends on the batch); X and vec(H) on the host."""
    from ace_amd import synth_problem, infer_low_rank_pipeline_batch, pipeline_cfg
    from ace_amd.engine import randperm
    from ace_amd.montecarlo import CHUNK
    from ace_amd.solver import VARIANTS
    assert count <= CHUNK
    cfg = pipeline_cfg(VARIANTS[method])
    R, mt = cfg.restarts, math.floor(M * cfg.cc_frac)
    A, B, _, H = synth_problem(SEED, 0, CHUNK, M, TX, RX, L=3, snr_db=30.0, device=gpu)
    tr = np.stack([np.stack([randperm(SEED, b * R + i, M, mt) for i in range(R)]) for b in range(CHUNK)])
    rec = infer_low_rank_pipeline_batch(A, B, TX, RX, tr, variant=method, restarts=R, maxiter=MAXITER)
    return rec.X[:count].cpu().numpy(), H[:count].cpu().numpy()


def _check_sweep(gpu, method, Ms):
    from ace_amd.montecarlo import vs_m
    out = vs_m(TX, RX, Ms, count=COUNT, method=method, maxiter=MAXITER, seed=SEED)
    nM = len(Ms)
    assert out["M"].tolist() == list(Ms)
    assert out["metrics"].shape == (nM, COUNT, 4) and out["status"].shape == (nM, COUNT)
    assert out["mean"].shape == (nM, 4) and out["n_degenerate"].shape == (nM,)
    assert np.isfinite(out["metrics"]).all() and np.isfinite(out["mean"]).all()
    np.testing.assert_allclose(out["mean"], out["metrics"].mean(axis=1), rtol=0, atol=1e-15)
    assert (out["n_degenerate"] == ((out["status"] & 256) != 0).sum(axis=1)).all()
    for k, M in enumerate(Ms):
        X, H = _recover(gpu, method, M, COUNT)
        live = (out["status"][k] & 256) == 0
        assert live.any()
        exp, nb = ER.evaluate(X[live], H[live], TX, RX)
        dev = np.abs(out["metrics"][k][live] - exp)
        gn = np.linalg.norm(H[live], axis=1)
        dev[:, 1] /= gn
        dev[:, 2] /= gn
        dev[nb, 1] = 0.0
        print(f"{method} M = {M}: mean {out['mean'][k]}, max deviation from the helper {dev.max(axis=0)}")
        assert (dev <= 1e-9).all(), (method, M, dev.max(axis=0))
    # shards compose: realisations 8..15 on their own
    part = vs_m(TX, RX, Ms, count=8, first=8, method=method, maxiter=MAXITER, seed=SEED)
    assert np.array_equal(part["metrics"], out["metrics"][:, 8:])
    assert np.array_equal(part["status"], out["status"][:, 8:])


def test_vs_m_a2only(gpu):
    _check_sweep(gpu, "A2only", [36, 64])


def test_shards_across_chunks_compose(gpu):
    """With chunks of 8 a shard solves other pipeline batches than the full run (the full run chunks 0 and 1, the
    shard of realisations 8..15 chunk 1 alone; the shard 4..11 both chunks, keeping half of each): the rows
    still agree bit for bit."""
    from ace_amd.montecarlo import vs_m
    kw = dict(method="A2only", maxiter=MAXITER, seed=SEED, chunk=8)
    full = vs_m(TX, RX, [64], count=16, **kw)
    for first, count in ((8, 8), (4, 8)):
        part = vs_m(TX, RX, [64], count=count, first=first, **kw)
        assert np.array_equal(part["metrics"], full["metrics"][:, first:first + count])
        assert np.array_equal(part["status"], full["status"][:, first:first + count])
    np.testing.assert_allclose(full["mean"], full["metrics"].mean(axis=1), rtol=0, atol=1e-15)


def test_vs_m_a2nuclear(gpu):
    _check_sweep(gpu, "A2nuclear", [64])


def test_refused_sweep_point_raises_the_pipeline_error(gpu):
    """floor(0.95 M) < min(20, M) train rows: the pipeline's own error, not a masked row
    (infer_low_rank_pipeline_batch reports a configuration its workspace query rejects as ValueError, a
    solve the library refuses as AceError)."""
    from ace_amd import AceError
    from ace_amd.montecarlo import vs_m
    with pytest.raises((AceError, ValueError)):
        vs_m(TX, RX, [4], count=4, seed=SEED, maxiter=MAXITER)
    with pytest.raises(ValueError):
        vs_m(TX, RX, [64], count=4, seed=SEED, method="phaselift")
    with pytest.raises(ValueError):
        vs_m(8, 4, [64], count=4, seed=SEED)   # (the synth's vec(H) order has rx leading: square arrays only)
