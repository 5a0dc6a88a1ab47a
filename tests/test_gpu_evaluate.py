"""GPU tests of the batched channel evaluator (ace_evaluate_*: Evaluation_H.m:73-132 on the device).

Target: the numpy restatement tests/eval_ref.py (numpy.linalg.svd in the beamformer's gauge) on seeded
inputs.  Bars: nmse and proj_err absolute 1e-9, the two gains 1e-9 ||G||_F -- a factor 10 over the 1e-10
the build holds on the singular vectors these are products of (tests/test_gpu_beamformer.py).  gain_ana
quantises phases: realisations in which the helper finds an entry of u1 or v1 within 1e-6 rad of a
quantisation boundary are left out of its comparison (a rounding-level phase difference legitimately flips
a code there), and at most 2 % of a shape's realisations may be left out.
"""
import functools
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import eval_ref as ER  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (8, 8), (16, 16), (25, 25), (26, 26), (32, 32), (32, 16), (16, 32)]
BATCHES = [1, 3, 65, 257]
ABS_BAR = 1e-9


@functools.lru_cache(maxsize=None)
def _problem(tx, rx):
    """257 seeded realisations of a shape with the helper's metrics: computed once, shared, never modified."""
    X, G = ER.seeded_problem(1000 * tx + rx, max(BATCHES), tx, rx)
    met, nb = ER.evaluate(X, G, tx, rx)
    for a in (X, G, met, nb):
        a.setflags(write=False)
    return X, G, met, nb


def _check(got, exp, G, nb, what):
    """The parity bars; returns the largest deviations (nmse, gain_ana / ||G||, gain_dig / ||G||, proj_err)."""
    gn = np.linalg.norm(G, axis=1)
    dev = np.abs(got - exp)
    dev[:, 1] /= gn
    dev[:, 2] /= gn
    dev[nb, 1] = 0.0
    worst = dev.max(axis=0)
    print(f"{what}: max deviation nmse {worst[0]:.2e} gain_ana {worst[1]:.2e} gain_dig {worst[2]:.2e} "
          f"proj_err {worst[3]:.2e} (gains over ||G||_F; {int(nb.sum())} near-boundary left out)")
    assert (worst <= ABS_BAR).all(), (what, worst, np.argwhere(dev > ABS_BAR)[:8])
    return worst


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("tx,rx", SHAPES, ids=[f"{t}x{r}" for t, r in SHAPES])
def test_parity_with_the_numpy_restatement(gpu, tx, rx, batch):
    from ace_amd import evaluate_host
    X, G, met, nb = _problem(tx, rx)
    assert nb.mean() <= 0.02, (tx, rx, int(nb.sum()))
    res = evaluate_host(X[:batch], G[:batch], tx, rx)
    assert (res.status == 0).all() and not res.degenerate.any()
    assert np.isfinite(res.metrics).all()
    np.testing.assert_array_equal(res.metrics[:, 0], res.nmse)
    np.testing.assert_array_equal(res.metrics[:, 3], res.proj_err)
    _check(res.metrics, met[:batch], G[:batch], nb[:batch], f"{tx}x{rx} batch {batch}")


@pytest.mark.parametrize("tx,rx", [(8, 8), (26, 26), (32, 16)])
def test_gauge_invariances(gpu, tx, rx):
    """A unit phase on x leaves nmse, gain_dig and proj_err unchanged; a power of j leaves gain_ana unchanged
    too (the same bars)."""
    from ace_amd import evaluate_host
    X, G, _, nb = _problem(tx, rx)
    X, G, nb = X[:65], G[:65], nb[:65]
    base = evaluate_host(X, G, tx, rx).metrics
    rng = np.random.default_rng(3)
    rot = evaluate_host(X * np.exp(2j * np.pi * rng.random((65, 1))), G, tx, rx).metrics
    everything = np.ones(65, bool)
    _check(rot, base, G, everything, f"{tx}x{rx} unit phase")        # (gain_ana left out for every row)
    for k in (1, 2, 3):
        _check(evaluate_host(X * 1j ** k, G, tx, rx).metrics, base, G, nb, f"{tx}x{rx} times j^{k}")


def test_degenerate_rows(gpu):
    """Row 1 of X zero, row 2 with a NaN, row 3 of G zero: flag and the stated values; every other row equals
    its value from the batch without them, bit for bit."""
    from ace_amd import evaluate_host
    from ace_amd._lib import ACE_ST_EVAL_DEGENERATE
    X, G, _, _ = _problem(8, 8)
    X, G = X[:6].copy(), G[:6].copy()
    clean = evaluate_host(X, G, 8, 8)
    X[1] = 0.0
    X[2, 17] = complex(np.nan, 0.0)
    G[3] = 0.0
    res = evaluate_host(X, G, 8, 8)
    assert res.degenerate.tolist() == [False, True, True, True, False, False]
    assert (res.status[[1, 2, 3]] == ACE_ST_EVAL_DEGENERATE).all() and (res.status[[0, 4, 5]] == 0).all()
    for b in (1, 2, 3):
        assert res.metrics[b].tolist() == [1.0, 0.0, 0.0, 1.0]
    for b in (0, 4, 5):
        assert np.array_equal(res.metrics[b], clean.metrics[b])
    inf = G.copy()
    inf[0, 3] = complex(0.0, -np.inf)
    assert evaluate_host(X, inf, 8, 8).degenerate.tolist() == [True, True, True, True, False, False]


def test_device_entry_on_a_stream_with_out(gpu):
    """evaluate_batch on a non-default stream into given outputs equals evaluate_host bit for bit."""
    import torch
    from ace_amd import evaluate_batch, evaluate_host, EvalResult
    X, G, _, _ = _problem(16, 32)
    host = evaluate_host(X, G, 16, 32)
    dX, dG = torch.from_numpy(X.copy()).to(gpu), torch.from_numpy(G.copy()).to(gpu)
    met = torch.full((len(X), 4), -1.0, dtype=torch.float64, device=gpu)
    st = torch.full((len(X),), -1, dtype=torch.int32, device=gpu)
    out = EvalResult(None, None, None, None, st, met)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=gpu)
    res = evaluate_batch(dX, dG, 16, 32, out=out, stream=s)
    s.synchronize()
    assert res.metrics.data_ptr() == met.data_ptr() and res.status.data_ptr() == st.data_ptr()
    assert np.array_equal(met.cpu().numpy(), host.metrics)
    assert np.array_equal(res.gain_ana.cpu().numpy(), host.gain_ana)
    assert np.array_equal(st.cpu().numpy().view(np.uint32), host.status)


def test_batch_invariance(gpu):
    """Batch 4096 at 32 x 32 equals the same rows evaluated in chunks of 1000, bit for bit."""
    import torch
    from ace_amd import evaluate_batch
    gen = torch.Generator(device=gpu).manual_seed(4096)
    G = torch.randn((4096, 1024), dtype=torch.complex128, device=gpu, generator=gen)
    X = G + 0.1 * torch.randn((4096, 1024), dtype=torch.complex128, device=gpu, generator=gen)
    full = evaluate_batch(X, G, 32, 32)
    parts = [evaluate_batch(X[i:i + 1000], G[i:i + 1000], 32, 32) for i in range(0, 4096, 1000)]
    torch.cuda.synchronize()
    assert torch.equal(full.metrics, torch.cat([p.metrics for p in parts]))
    assert torch.equal(full.status, torch.cat([p.status for p in parts]))
    assert (full.status == 0).all() and torch.isfinite(full.metrics).all()
