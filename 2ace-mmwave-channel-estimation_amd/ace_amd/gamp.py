"""Batched EM-BG-GAMP on the GPU (``ace_gamp_solve_*``, csrc/ace_gamp.hip): the sparse solver of the two-stage
PLGAMP recovery (My_TwoStage_Recovery.m:163-181) and the first branch of My_Conventional_CS.m:79.

The reference vendors the solver under ``main/3rd_software_component/GAMP/trunk/code`` (``EMGMAMP/EMBGAMP.m``,
``EMGMAMP/EMGMAMP.m``, ``main/gampEst.m`` and the estimators ``CAwgnEstimIn``, ``CAwgnEstimOut``, ``SparseScaEstim``);
the kernel restates it for the two option sets the reference uses (they differ in ``learn_lambda`` only), one column
per realisation, against one shared dictionary ``D`` [d][N].  Expectation-maximisation over a Bernoulli-Gaussian
prior (sparsity rate lambda, active variance phi, mean 0) and the noise variance psi, around generalised approximate
message passing with adaptive damping; include/ace.h and the kernel's header state the iteration and the quirks of
the reference that decide its trajectory.

A realisation with a non-finite ``y`` returns zeros and ACE_ST_EVAL_DEGENERATE.  Where the reference would raise
(its callers catch that and run OMP) the realisation returns zeros and ACE_ST_GAMP_FAILED; ``sparse.plgamp_batch``
is the caller that runs the OMP fallback.

Entry points (no CPU fallback -- every call runs ``gamp_kernel`` on the GPU):
  * ``embgamp_host(D, Y, snr_db, lam, ...)``  -- numpy arrays.
  * ``embgamp_batch(D, Y, snr_db, lam, ...)`` -- device tensors already in HBM; no host copy.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import (LIB, check, gamp_cfg, ACE_ST_EVAL_DEGENERATE, ACE_ST_GAMP_FAILED, ACE_ST_GAMP_MAXEM,
                   ACE_ST_GAMP_NANBREAK)

D_MAX, N_MAX = 256, 16384   # the C-ABI's limits (include/ace.h)


@dataclass
class GampResult:
    xhat: object       # [batch][N] complex128, the posterior means of the final GAMP call
    params: object     # [batch][3] float64: lambda, phi, psi at exit
    em_iters: object   # [batch] int32, EM iterations started
    status: object     # [batch] uint32 (host) / int32 (device)
    trace: object = None   # [batch][max_em_iter + 1][2] int32 (iterations, pass mask) per GAMP call, or None
    xvar: object = None    # [batch][N] float64 posterior variances, or None when not requested

    @property
    def failed(self):
        return (self.status & ACE_ST_GAMP_FAILED) != 0

    @property
    def degenerate(self):
        return (self.status & ACE_ST_EVAL_DEGENERATE) != 0

    @property
    def nan_break(self):
        return (self.status & ACE_ST_GAMP_NANBREAK) != 0

    @property
    def max_em(self):
        return (self.status & ACE_ST_GAMP_MAXEM) != 0

    def channel(self, AD):
        """``AD @ xhat`` per realisation ([batch][rows of AD]), as ``OmpResult.channel`` (Recover_Channel.m:
        AD * plgamp_signal)."""
        if isinstance(self.xhat, np.ndarray):
            return self.xhat @ np.asarray(AD).T
        return (self.xhat @ AD.transpose(0, 1)).contiguous()


def _shapes(ds, ys):
    if len(ds) != 2 or not 1 <= ds[0] <= D_MAX or not 1 <= ds[1] <= N_MAX:
        raise ValueError(f"D must be [d][N] with 1 <= d <= {D_MAX} and 1 <= N <= {N_MAX}, got {tuple(ds)}")
    d, N = ds
    if len(ys) != 2 or ys[0] < 1 or ys[1] != d:
        raise ValueError(f"Y must be [batch][d] = [batch][{d}], got {tuple(ys)}")
    return ys[0], d, N


def _cfg(snr_db, lam, learn_lambda, max_em_iter, cfg_kw):
    return gamp_cfg(snr_db=float(snr_db), lambda0=float(lam), learn_lambda=int(bool(learn_lambda)),
                    max_em_iter=int(max_em_iter), **cfg_kw)


def embgamp_host(D, Y, snr_db, lam, *, learn_lambda=False, max_em_iter=200, trace=False, want_xvar=False,
                 **cfg_kw) -> GampResult:
    """EM-BG-GAMP for a batch on host arrays (see the module text).  ``cfg_kw``: further ``ace_gamp_cfg`` fields
    (gamp_nit, step0, gamp_tol)."""
    D = np.ascontiguousarray(np.atleast_2d(np.asarray(D, dtype=np.complex128)))
    Y = np.ascontiguousarray(np.atleast_2d(np.asarray(Y, dtype=np.complex128)))
    batch, d, N = _shapes(D.shape, Y.shape)
    cfg = _cfg(snr_db, lam, learn_lambda, max_em_iter, cfg_kw)
    xhat = np.empty((batch, N), np.complex128)
    xvar = np.empty((batch, N), np.float64) if want_xvar else None
    par = np.empty((batch, 3), np.float64)
    emi = np.empty(batch, np.int32)
    tr = np.empty((batch, cfg.max_em_iter + 1, 2), np.int32) if trace else None
    st = np.empty(batch, np.uint32)
    dp = lambda a: None if a is None else a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    check(LIB.ace_gamp_solve_host(C.byref(cfg), batch, d, N, dp(D), dp(Y), dp(xhat), dp(xvar), dp(par), ip(emi), ip(tr),
                                  st.ctypes.data_as(C.POINTER(C.c_uint32))))
    return GampResult(xhat, par, emi, st, tr, xvar)


def embgamp_batch(D, Y, snr_db, lam, *, learn_lambda=False, max_em_iter=200, trace=False, want_xvar=False,
                  workspace=None, stream=None, **cfg_kw) -> GampResult:
    """EM-BG-GAMP on device tensors: D [d][N] and Y [batch][d] complex128; ``snr_db`` initialises the noise variance
    and ``lam`` the sparsity rate (s / n at both of the reference's call sites).  Asynchronous on ``stream`` (default:
    the current stream); nothing is copied to the host.  ``workspace``: a ``solver.Workspace`` to take the state
    vectors from (default: the package's shared one)."""
    import torch
    from .solver import _DEFAULT_WS
    if not (D.is_cuda and Y.is_cuda):
        raise ValueError("embgamp_batch needs device tensors")
    if D.dtype != torch.complex128 or Y.dtype != torch.complex128:
        raise TypeError("D and Y must be complex128")
    batch, d, N = _shapes(tuple(D.shape), tuple(Y.shape))
    dev = D.device
    if Y.device != dev:
        raise ValueError("D and Y must be on one device")
    cfg = _cfg(snr_db, lam, learn_lambda, max_em_iter, cfg_kw)
    D, Y = D.contiguous(), Y.contiguous()
    xhat = torch.empty((batch, N), dtype=torch.complex128, device=dev)
    xvar = torch.empty((batch, N), dtype=torch.float64, device=dev) if want_xvar else None
    par = torch.empty((batch, 3), dtype=torch.float64, device=dev)
    emi = torch.empty(batch, dtype=torch.int32, device=dev)
    tr = torch.empty((batch, cfg.max_em_iter + 1, 2), dtype=torch.int32, device=dev) if trace else None
    st = torch.empty(batch, dtype=torch.int32, device=dev)
    nbytes = int(LIB.ace_gamp_workspace_size(batch, d, N)) + 256
    ws = (workspace or _DEFAULT_WS).get(nbytes, dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    check(LIB.ace_gamp_solve_batch(C.byref(cfg), batch, d, N, D.data_ptr(), Y.data_ptr(), xhat.data_ptr(), ptr(xvar),
                                   par.data_ptr(), emi.data_ptr(), ptr(tr), st.data_ptr(), ws.data_ptr(), ws.numel(),
                                   stream.cuda_stream))
    return GampResult(xhat, par, emi, st, tr, xvar)
