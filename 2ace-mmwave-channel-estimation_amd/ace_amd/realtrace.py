"""Measured RSS traces: the sweep over the number of training probes and the closed-loop tracker, scored
on held-out probes (``rss.evaluate_rss_batch``, the reference's ``Evaluate_rss``) since a real trace has no
true H to compare with.

``vs_m``  -- Numerical_Simulation/main_programs/VS_M_real_rss.m: recover from M training probes for each M
of a sweep, score every recovery on the test probes.  ``track`` -- RSS_Mobility_simu.m:131-165: a sliding
window of probes is recovered every time slot, scored on the slot's unused probes, and the score decides
how many probes the next slot spends (``next_m``).

Codebook, RSS and estimates stay on the device; per sweep point only the [T][4] metrics and the status
words come back (``track``: one scalar per slot, because the next window's shape depends on it).

Chunks.  As in ``montecarlo.vs_m`` the pipeline's results depend, at rounding level, on the batch a
realisation is solved in, so ``vs_m`` always solves trace t of the full run in chunk ``t // chunk``: a call
on a subset of the traces (``first`` = the full-run index of its first trace, a multiple of ``chunk``)
reproduces its rows of the full run bit for bit, provided the subset ends on a chunk boundary or at the
end of the full run.
"""
from __future__ import annotations

import math

import numpy as np

from ._lib import pipeline_cfg
from .engine import RSS_FCT, randperm
from .montecarlo import CHUNK, METHODS
from .rss import METRICS, dbm_to_amp, evaluate_rss_batch


# ---------------------------------------------------------------- pure helpers (no GPU)
def split_rows(P, test_rows=None, n_test=None):
    """(pool, test) row indices of a P-row codebook: ``test_rows`` (an index array) or the last ``n_test`` rows
    are held out -- exactly one of the two is given -- and the remaining rows are the training pool in their
    given order."""
    P = int(P)
    if (test_rows is None) == (n_test is None):
        raise ValueError("give exactly one of test_rows and n_test")
    if n_test is not None:
        n_test = int(n_test)
        if not 1 <= n_test < P:
            raise ValueError(f"n_test must be in 1..{P - 1}, got {n_test}")
        test = np.arange(P - n_test, P, dtype=np.int64)
    else:
        test = np.asarray(test_rows, dtype=np.int64).reshape(-1)
        if test.size < 1 or test.min() < 0 or test.max() >= P or np.unique(test).size != test.size:
            raise ValueError(f"test_rows must be distinct indices in 0..{P - 1}")
    held = np.zeros(P, bool)
    held[test] = True
    pool = np.nonzero(~held)[0].astype(np.int64)
    if pool.size < 1:
        raise ValueError("no training rows left")
    return pool, test


def train_rows(pool, M, k, rows="first", seed=0, cb=None):
    """The M training rows of sweep point k: ``rows="first"`` the pool's first M (picked_beams = 1:M,
    Generate_Sensing_Matrix_with_candidate.m:12); ``rows="randperm"`` pool[engine.randperm(seed, k, len(pool), M)]
    (the drivers' choice); ``rows="aopt"`` the Bayesian A-optimal choice among the pool's rows of the codebook ``cb``
    [P][n] (the 'Bayes_Beam' mode, :14: ``design.bayes_beam(cb, M, seed=seed, stream_id=k, candidates=pool)``, on the
    GPU; a row may come back more than once, as in the reference)."""
    pool = np.asarray(pool, dtype=np.int64)
    M = int(M)
    if not 1 <= M <= pool.size:
        raise ValueError(f"M must be in 1..{pool.size} (the training pool), got {M}")
    if rows == "first":
        return pool[:M].copy()
    if rows == "randperm":
        return pool[randperm(seed, k, pool.size, M).astype(np.int64)]
    if rows == "aopt":
        if cb is None:
            raise ValueError("rows='aopt' needs the codebook cb")
        from .design import bayes_beam
        dev = cb.device if hasattr(cb, "device") and not isinstance(cb, np.ndarray) else None
        return bayes_beam(cb, M, seed=seed, stream_id=k, candidates=pool, device=dev)
    raise ValueError(f"rows must be 'first', 'randperm' or 'aopt', got {rows!r}")


def next_m(M, err, m_max=80, threshold=0.2):
    """RSS_Mobility_simu.m:158-162: spend fewer probes in the next slot when the held-out error is below the
    threshold (M - floor(M/5) - 1, not below 0), more otherwise (M + floor(M/5) + 1, capped at m_max)."""
    M = int(M)
    step = M // 5 + 1
    return max(0, M - step) if err < threshold else min(int(m_max), M + step)


def _cfg(method):
    from .solver import VARIANTS
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    return pipeline_cfg(VARIANTS[method])


def _device_inputs(cb, rss_dbm, tx, rx, rss_fct, device):
    import torch
    dev = torch.device("cuda" if device is None else device)
    host = lambda a: np.array(a) if isinstance(a, np.ndarray) else a   # noqa: E731  (a copy: the input may be read-only)
    cb = torch.as_tensor(host(cb), device=dev).to(torch.complex128)
    amp = dbm_to_amp(torch.as_tensor(host(rss_dbm), device=dev), rss_fct)
    if cb.dim() != 2 or cb.shape[1] != tx * rx:
        raise ValueError(f"cb must be [P][tx*rx] = [P][{tx * rx}], got {tuple(cb.shape)}")
    return dev, cb, amp


# ---------------------------------------------------------------- VS_M_real_rss
def vs_m(cb, rss_dbm, tx, rx, M_list, *, test_rows=None, n_test=None, rows="first", method="A2only", seed,
         maxiter=None, rss_fct=RSS_FCT, chunk=CHUNK, device=None, first=0, return_X=False) -> dict:
    """Held-out RSS error of the recoveries from M training probes, for each M of ``M_list``.

    ``cb`` [P][n] complex, ``rss_dbm`` [T][P] or [P]: T traces measured with the same codebook (the
    reference's repeated rounds), in dBm.  The rows are split once (``split_rows``); sweep point k trains on
    ``train_rows(pool, M, k, rows, seed)``: A = cb[those rows], B = ``dbm_to_amp`` of their RSS.  Trace b of
    the call is trace ``first + b`` of the full run; its train partitions come from the build's counter RNG,
    ``engine.randperm(seed, (first + b) * restarts + restart, M, floor(cc_frac M))``, as ``montecarlo.vs_m``
    draws them, and it is solved in chunk ``(first + b) // chunk`` (``first`` must be a multiple of ``chunk``;
    see the module text).  ``maxiter`` caps every ADMM stage (default: the reference's 500).

    Returns a dict: ``M`` [nM], ``metrics`` [nM][T][4] (columns ``rss.METRICS``), ``status`` [nM][T] (the
    evaluator's), ``mean`` [nM][4] (over the traces; degenerate ones count with 1, 1, 1, 0), ``rows`` (list of
    the training rows per sweep point), ``test_rows``; with ``return_X`` also ``X``, the estimates
    [nM][T][n] as a device tensor.  A sweep point the pipeline refuses raises the pipeline's own error."""
    import torch
    from .pipeline import infer_low_rank_pipeline_batch
    cfg = _cfg(method)
    R = cfg.restarts
    first, chunk = int(first), int(chunk)
    if chunk < 1 or first < 0 or first % chunk:
        raise ValueError("chunk must be >= 1 and first a non-negative multiple of chunk")
    dev, cb, amp = _device_inputs(cb, rss_dbm, tx, rx, rss_fct, device)
    if amp.dim() == 1:
        amp = amp[None]
    P = cb.shape[0]
    if amp.dim() != 2 or amp.shape[1] != P:
        raise ValueError(f"rss_dbm must be [T][P] or [P] with P = {P}, got {tuple(amp.shape)}")
    T = amp.shape[0]
    pool, test = split_rows(P, test_rows, n_test)
    Ms = [int(M) for M in M_list]
    kw = {} if maxiter is None else {"maxiter": int(maxiter)}
    cb_test = cb[torch.as_tensor(test, device=dev)].contiguous()
    rss_test = amp[:, torch.as_tensor(test, device=dev)].contiguous()
    metrics = np.empty((len(Ms), T, 4), np.float64)
    status = np.empty((len(Ms), T), np.uint32)
    used, Xs = [], []
    for k, M in enumerate(Ms):
        rk = train_rows(pool, M, k, rows, seed, cb=cb)
        used.append(rk)
        ridx = torch.as_tensor(rk, device=dev)
        A = cb[ridx].contiguous()
        B = amp[:, ridx].contiguous()
        mt = math.floor(M * cfg.cc_frac)
        Xk = []
        for c0 in range(0, T, chunk):
            c1 = min(T, c0 + chunk)
            tr = np.stack([np.stack([randperm(seed, (first + b) * R + i, M, mt) for i in range(R)])
                           for b in range(c0, c1)])
            rec = infer_low_rank_pipeline_batch(A, B[c0:c1], tx, rx, tr, variant=method, restarts=R, **kw)
            ev = evaluate_rss_batch(rec.X, cb_test, rss_test[c0:c1])
            metrics[k, c0:c1] = ev.metrics.cpu().numpy()
            status[k, c0:c1] = ev.status.cpu().numpy().view(np.uint32)
            if return_X:
                Xk.append(rec.X)
        if return_X:
            Xs.append(torch.cat(Xk))
    out = {"M": np.asarray(Ms, np.int64), "metrics": metrics, "status": status, "mean": metrics.mean(axis=1),
           "rows": used, "test_rows": test, "columns": METRICS}
    if return_X:
        out["X"] = torch.stack(Xs) if Xs else None
    return out


# ---------------------------------------------------------------- RSS_Mobility_simu
def track(cb, rss_dbm, tx, rx, *, slot=100, m_max=80, keep=400, threshold=0.2, method="A2only", seed,
          maxiter=None, rss_fct=RSS_FCT, device=None) -> dict:
    """The closed loop of RSS_Mobility_simu.m:131-165 for one trace of P = Tw * slot probes in time order.

    Slot t (0-based) spends M_t probes: its first M_t rows join the sliding window, which keeps its last
    ``keep + 1`` entries (the reference's ``max(numel - 400, 1):numel`` keeps 401 of them: restated as it
    stands); the window is recovered as a batch of one with a train partition per restart from
    ``engine.randperm(seed, t * restarts + restart, W, floor(cc_frac W))`` (W the window's length), and the
    recovery is scored by ``evaluate_rss_batch`` on the slot's remaining ``slot - M_t`` probes.
    M_{t+1} = ``next_m(M_t, score, m_max, threshold)``, M_0 = m_max.  M_t = 0 is legal: nothing is appended
    and the whole slot is the test set.  A slot with M_t = slot has no test rows: it keeps M and records NaN.

    Departure from the reference script, which hands ``db2pow(rss_trace)`` (a power) to the solver and to
    Evaluate_rss without the square root: the trace is converted like the drivers', through ``dbm_to_amp``.

    Returns a dict: ``M`` [Tw] int64, ``mean_rel`` [Tw] float64, ``status`` [Tw] uint32 (the evaluator's; 0
    for a slot that was not scored)."""
    import torch
    from .pipeline import infer_low_rank_pipeline_batch
    cfg = _cfg(method)
    R = cfg.restarts
    slot, m_max, keep = int(slot), int(m_max), int(keep)
    if slot < 1 or not 1 <= m_max <= slot or keep < 0:
        raise ValueError("need slot >= 1, 1 <= m_max <= slot and keep >= 0")
    dev, cb, amp = _device_inputs(cb, rss_dbm, tx, rx, rss_fct, device)
    P = cb.shape[0]
    if amp.dim() != 1 or amp.shape[0] != P or P % slot:
        raise ValueError(f"rss_dbm must be [P] with P = {P} a multiple of slot = {slot}, got {tuple(amp.shape)}")
    Tw = P // slot
    kw = {} if maxiter is None else {"maxiter": int(maxiter)}
    Ms = np.zeros(Tw, np.int64)
    score = np.full(Tw, np.nan)
    sts = [None] * Tw
    window = np.zeros(0, np.int64)
    M = m_max
    for t in range(Tw):
        Ms[t] = M
        window = np.concatenate([window, slot * t + np.arange(M, dtype=np.int64)])[-(keep + 1):]
        if M == slot:
            continue
        W = window.size
        mt = math.floor(W * cfg.cc_frac)
        tr = np.stack([randperm(seed, t * R + i, W, mt) for i in range(R)])
        widx = torch.as_tensor(window, device=dev)
        rec = infer_low_rank_pipeline_batch(cb[widx].contiguous(), amp[widx][None].contiguous(), tx, rx, tr,
                                            variant=method, restarts=R, **kw)
        ev = evaluate_rss_batch(rec.X, cb[slot * t + M:slot * (t + 1)], amp[slot * t + M:slot * (t + 1)])
        sts[t] = ev.status
        score[t] = float(ev.mean_rel[0])   # the one scalar per slot that has to reach the host
        M = next_m(M, score[t], m_max, threshold)
    status = np.zeros(Tw, np.uint32)
    live = [t for t in range(Tw) if sts[t] is not None]
    if live:
        status[live] = torch.cat([sts[t] for t in live]).cpu().numpy().view(np.uint32)
    return {"M": Ms, "mean_rel": score, "status": status}
