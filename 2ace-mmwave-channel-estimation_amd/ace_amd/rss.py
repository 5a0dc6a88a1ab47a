"""Held-out RSS evaluation on the GPU: the reference's ``Evaluate_rss``
(main/src/evaluate_plot_results/Evaluate_rss.m and its copy under Numerical_Simulation), batched::

    rss_eval   = abs(cb_test * H)
    Evaluation = mean(abs(rss_eval - rss_test) ./ rss_test)

The score a testbed user can form without the true channel: predict the RSS of probes that were held out
of the recovery and compare with what was measured.  Per realisation, over the usable test rows p
(``rel_p = | |cb_test[p] . x| - rss_p | / rss_p``, no conjugate on the codebook):
  * ``mean_rel`` -- the reference's ``Evaluation``,
  * ``rms_rel``, ``max_rel`` -- root mean square and maximum of the same per-row values,
  * ``n_used``   -- the number of usable rows.
``rss_test`` holds measured AMPLITUDES in X's units (``dbm_to_amp``), not dBm.  A row whose rss is not
finite or <= 0 is left out and flagged ACE_ST_RSS_SKIPPED; a realisation whose X has a non-finite entry,
or that has no usable row, returns 1, 1, 1, n_used = 0 and ACE_ST_EVAL_DEGENERATE (the reference gives Inf
or NaN in both cases).  An all-zero X is not degenerate: it predicts 0 and scores 1.

Entry points (no CPU fallback -- every call runs ``rsseval_kernel`` on the GPU):
  * ``evaluate_rss_host(X, cb_test, rss_test)`` -- numpy arrays.
  * ``evaluate_rss_batch(X, cb_test, rss_test)`` -- device tensors already in HBM; no host copy.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import LIB, check, ACE_ST_EVAL_DEGENERATE, ACE_ST_RSS_SKIPPED
from .engine import RSS_FCT

METRICS = ("mean_rel", "rms_rel", "max_rel", "n_used")   # column order of the C-ABI's metrics [batch][4]


@dataclass
class RssEval:
    mean_rel: object   # [batch] float64
    rms_rel: object    # [batch] float64
    max_rel: object    # [batch] float64
    n_used: object     # [batch] float64 (a count)
    status: object     # [batch] uint32 (host) / int32 (device): ACE_ST_RSS_SKIPPED, ACE_ST_EVAL_DEGENERATE
    metrics: object = None   # [batch][4], the four columns above as one array (views)
    pred: object = None      # [batch][Pt] float64 |cb_test x_b|, or None when not requested

    @property
    def degenerate(self):
        return (self.status & ACE_ST_EVAL_DEGENERATE) != 0

    @property
    def skipped(self):
        return (self.status & ACE_ST_RSS_SKIPPED) != 0


def _result(metrics, status, pred) -> RssEval:
    return RssEval(metrics[:, 0], metrics[:, 1], metrics[:, 2], metrics[:, 3], status, metrics, pred)


def _shapes(xs, cs, rs):
    """(batch, n, Pt, rss_shared) of X [batch][n], cb_test [Pt][n], rss_test [Pt] or [batch][Pt]."""
    if len(xs) != 2 or len(cs) != 2 or cs[1] != xs[1] or xs[0] < 1 or xs[1] < 1 or cs[0] < 1:
        raise ValueError(f"X must be [batch][n] and cb_test [Pt][n], got {tuple(xs)} and {tuple(cs)}")
    batch, n, Pt = xs[0], xs[1], cs[0]
    if tuple(rs) == (Pt,):
        return batch, n, Pt, 1
    if tuple(rs) == (batch, Pt):
        return batch, n, Pt, 0
    raise ValueError(f"rss_test must be [Pt] = [{Pt}] or [batch][Pt] = [{batch}][{Pt}], got {tuple(rs)}")


def dbm_to_amp(rss_dbm, rss_fct=RSS_FCT):
    """Measured RSS in dBm -> the amplitudes the recovery works in: sqrt(10^(dBm/10) / 1000) * rss_fct
    (channel_recovery_ADMM_v2_simulation_A2only.m:139, VS_M_real_rss.m:164-165).  numpy arrays or tensors."""
    try:
        import torch
        if isinstance(rss_dbm, torch.Tensor):
            return torch.sqrt(torch.pow(10.0, rss_dbm.to(torch.float64) / 10.0) / 1000.0) * float(rss_fct)
    except ImportError:   # (numpy-only callers)
        pass
    return np.sqrt(np.power(10.0, np.asarray(rss_dbm, dtype=np.float64) / 10.0) / 1000.0) * float(rss_fct)


def evaluate_rss_host(X, cb_test, rss_test, *, want_pred=False) -> RssEval:
    """Evaluate_rss for a batch on host arrays: X [batch][n] (estimates), cb_test [Pt][n] complex, rss_test
    [Pt] (shared by the batch) or [batch][Pt] measured amplitudes."""
    X = np.ascontiguousarray(np.atleast_2d(np.asarray(X, dtype=np.complex128)))
    cb = np.ascontiguousarray(np.atleast_2d(np.asarray(cb_test, dtype=np.complex128)))
    rs = np.ascontiguousarray(np.asarray(rss_test, dtype=np.float64))
    batch, n, Pt, shared = _shapes(X.shape, cb.shape, rs.shape)
    met = np.empty((batch, 4), np.float64)
    st = np.empty(batch, np.uint32)
    pred = np.empty((batch, Pt), np.float64) if want_pred else None
    dp = lambda a: a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    check(LIB.ace_rss_evaluate_host(batch, n, Pt, dp(X), dp(cb), dp(rs), shared, dp(met),
                                    dp(pred) if want_pred else None, st.ctypes.data_as(C.POINTER(C.c_uint32))))
    return _result(met, st, pred)


def evaluate_rss_batch(X, cb_test, rss_test, *, want_pred=False, out=None, stream=None) -> RssEval:
    """Evaluate_rss on device tensors: X [batch][n], cb_test [Pt][n] complex128, rss_test [Pt] or [batch][Pt]
    float64.  ``out``: an RssEval of an earlier call with the same batch and Pt (its ``metrics`` [batch][4]
    float64, ``status`` [batch] int32 and, with ``want_pred``, ``pred`` [batch][Pt] float64 tensors are
    reused).  Asynchronous on ``stream`` (default: the current stream); nothing is copied to the host."""
    import torch
    if not (X.is_cuda and cb_test.is_cuda and rss_test.is_cuda):
        raise ValueError("evaluate_rss_batch needs device tensors")
    if X.dtype != torch.complex128 or cb_test.dtype != torch.complex128:
        raise TypeError("X and cb_test must be complex128")
    if rss_test.dtype != torch.float64:
        raise TypeError("rss_test must be float64")
    batch, n, Pt, shared = _shapes(tuple(X.shape), tuple(cb_test.shape), tuple(rss_test.shape))
    dev = X.device
    if cb_test.device != dev or rss_test.device != dev:
        raise ValueError("X, cb_test and rss_test must be on one device")
    X, cb_test, rss_test = X.contiguous(), cb_test.contiguous(), rss_test.contiguous()
    if out is None:
        met = torch.empty((batch, 4), dtype=torch.float64, device=dev)
        st = torch.empty(batch, dtype=torch.int32, device=dev)
        pred = torch.empty((batch, Pt), dtype=torch.float64, device=dev) if want_pred else None
    else:
        met, st, pred = out.metrics, out.status, out.pred if want_pred else None
        if (tuple(met.shape) != (batch, 4) or met.dtype != torch.float64 or not met.is_contiguous()
                or tuple(st.shape) != (batch,) or st.dtype != torch.int32 or met.device != dev or st.device != dev):
            raise ValueError("out must hold metrics [batch][4] float64 and status [batch] int32 on X's device")
        if want_pred and (pred is None or tuple(pred.shape) != (batch, Pt) or pred.dtype != torch.float64
                          or not pred.is_contiguous() or pred.device != dev):
            raise ValueError("out must hold pred [batch][Pt] float64 on X's device when want_pred is set")
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    check(LIB.ace_rss_evaluate_batch(batch, n, Pt, X.data_ptr(), cb_test.data_ptr(), rss_test.data_ptr(), shared,
                                     met.data_ptr(), pred.data_ptr() if want_pred else None, st.data_ptr(),
                                     stream.cuda_stream))
    return _result(met, st, pred)
