"""Batched min-L2 ADMM on the GPU (``ace_minl2_*``, csrc/ace_minl2.hip): ``Method.ADMM`` of the reference's Vs_M
figure, i.e. ``ADMM_v2(..., version 0)`` -> ``inferMinL2.m``, the 2ACE ADMM with the low-rank Z-block taken out --
minimise ``|| |A X| - B ||`` with ``X = pinv(A) (Y - M / mu)``.  It is the curve that shows what the rank prior buys.

``infer_min_l2_host`` / ``infer_min_l2_batch`` run the whole of ``inferMinL2`` for a batch sharing one ``A`` and one
train partition: normalisation, the 95 / 5 partition (m_t = ceil(0.95 m)), the spectral initialisation with its
per-realisation column count, the row-form and per-column stages, the quality on the test rows, the r = 1 refinement
on the full ``A`` where the quality exceeds 0.6, and the rollback.  ``inferMinL2(A, B)`` is the MATLAB calling style.

``minl2_admm_host`` / ``minl2_admm_batch`` run one ``InferADMM`` call (inferMinL2.m:229-326, lambda = 0) for a batch
of realisations against one shared ``A``: the initialisation and every iteration in one kernel launch, the three
m x n products of an iteration on the f64 matrix cores.  include/ace.h states the shapes, the limits and the
departures (a rank-deficient ``A`` raises ``AceError`` with ACE_ERR_UNSUPPORTED where MATLAB's pinv would truncate).

There is no CPU fallback: every call runs ``minl2_kernel`` on the GPU.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from ._lib import LIB, check, minl2_cfg, ACE_ST_CONVERGED, ACE_ST_NO_OPT, ACE_ST_ROLLBACK

N_MAX, M_MAX, R_MAX = 1024, 4096, 32   # the C-ABI's limits (include/ace.h)


@dataclass
class MinL2Stage:
    """One InferADMM call.  Row form: X [batch][r][n], Y [batch][r][m]; per-column form: X [batch][n], Y [batch][m]."""
    X: object
    Y: object
    iters: object      # [batch] int32, iterations run
    objcol: object     # [batch] int32, the column returned (0 in the row form)
    opt_obj: object    # [batch] float64, the best objective || |A X| - B ||
    mu: object         # [batch] float64 at exit
    status: object     # [batch] uint32 (host) / int32 (device)
    Xall: object = None   # [batch][r][n]: every column of the iterate at the best iteration, or None

    @property
    def converged(self):
        return (self.status & ACE_ST_CONVERGED) != 0

    @property
    def no_opt(self):
        return (self.status & ACE_ST_NO_OPT) != 0


def _shapes(a, b, x0):
    if len(a) != 2 or not 1 <= a[0] <= M_MAX or not 1 <= a[1] <= N_MAX:
        raise ValueError(f"A must be [m][n] with 1 <= m <= {M_MAX} and 1 <= n <= {N_MAX}, got {tuple(a)}")
    m, n = a
    if len(b) != 2 or b[0] < 1 or b[1] != m:
        raise ValueError(f"B must be [batch][m] = [batch][{m}], got {tuple(b)}")
    if len(x0) != 3 or x0[0] != b[0] or not 1 <= x0[1] <= R_MAX or x0[2] != n:
        raise ValueError(f"X0 must be [batch][r][n] = [{b[0]}][1..{R_MAX}][{n}], got {tuple(x0)}")
    return b[0], m, n, x0[1]


def _cfg(maxiter, cfg_kw):
    return minl2_cfg(maxiter=int(maxiter), **cfg_kw)


def minl2_admm_host(A, B, X0, *, scale_by_row, rcols=None, maxiter=500, want_xall=False, **cfg_kw) -> MinL2Stage:
    """One InferADMM call on host arrays: A [m][n], B [batch][m], X0 [batch][r][n] (column j of realisation b at
    ``X0[b, j]``), ``rcols`` [batch] the columns that exist per realisation (default r).  ``cfg_kw``: further
    ``ace_minl2_cfg`` fields (mu0, rho, tol_rel, tol_abs)."""
    A = np.ascontiguousarray(np.asarray(A, dtype=np.complex128))
    B = np.ascontiguousarray(np.atleast_2d(np.asarray(B, dtype=np.float64)))
    X0 = np.ascontiguousarray(np.asarray(X0, dtype=np.complex128))
    batch, m, n, r = _shapes(A.shape, B.shape, X0.shape)
    rc = None if rcols is None else np.ascontiguousarray(np.asarray(rcols, dtype=np.int32))
    if rc is not None and rc.shape != (batch,):
        raise ValueError(f"rcols must be [batch] = [{batch}], got {rc.shape}")
    cfg = _cfg(maxiter, cfg_kw)
    ro = (batch, r) if scale_by_row else (batch,)
    X = np.empty(ro + (n,), np.complex128)
    Y = np.empty(ro + (m,), np.complex128)
    Xall = np.empty((batch, r, n), np.complex128) if want_xall else None
    it = np.empty(batch, np.int32)
    oc = np.empty(batch, np.int32)
    obj = np.empty(batch, np.float64)
    mu = np.empty(batch, np.float64)
    st = np.empty(batch, np.uint32)
    dp = lambda a: None if a is None else a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    check(LIB.ace_minl2_admm_host(C.byref(cfg), batch, m, n, r, int(bool(scale_by_row)), dp(A), dp(B), dp(X0), ip(rc),
                                  dp(X), dp(Y), dp(Xall), ip(it), ip(oc), dp(obj), dp(mu),
                                  st.ctypes.data_as(C.POINTER(C.c_uint32))))
    return MinL2Stage(X, Y, it, oc, obj, mu, st, Xall)


def minl2_admm_batch(A, B, X0, *, scale_by_row, rcols=None, maxiter=500, want_xall=False, workspace=None, stream=None,
                     **cfg_kw) -> MinL2Stage:
    """One InferADMM call on device tensors: A [m][n] and X0 [batch][r][n] complex128, B [batch][m] float64, ``rcols``
    [batch] int32 or None.  Synchronises ``stream`` once (the pivot test of pinv's setup), nothing else is copied to the
    host.  ``workspace``: a ``solver.Workspace`` (default: the package's shared one)."""
    import torch
    from .solver import _DEFAULT_WS
    if not (A.is_cuda and B.is_cuda and X0.is_cuda):
        raise ValueError("minl2_admm_batch needs device tensors")
    if A.dtype != torch.complex128 or X0.dtype != torch.complex128 or B.dtype != torch.float64:
        raise TypeError("A and X0 must be complex128, B float64")
    batch, m, n, r = _shapes(tuple(A.shape), tuple(B.shape), tuple(X0.shape))
    dev = A.device
    if B.device != dev or X0.device != dev or (rcols is not None and rcols.device != dev):
        raise ValueError("A, B, X0 and rcols must be on one device")
    if rcols is not None and (rcols.dtype != torch.int32 or tuple(rcols.shape) != (batch,)):
        raise TypeError(f"rcols must be int32 [batch] = [{batch}]")
    cfg = _cfg(maxiter, cfg_kw)
    A, B, X0 = A.contiguous(), B.contiguous(), X0.contiguous()
    rc = None if rcols is None else rcols.contiguous()
    ro = (batch, r) if scale_by_row else (batch,)
    X = torch.empty(ro + (n,), dtype=torch.complex128, device=dev)
    Y = torch.empty(ro + (m,), dtype=torch.complex128, device=dev)
    Xall = torch.empty((batch, r, n), dtype=torch.complex128, device=dev) if want_xall else None
    it = torch.empty(batch, dtype=torch.int32, device=dev)
    oc = torch.empty(batch, dtype=torch.int32, device=dev)
    obj = torch.empty(batch, dtype=torch.float64, device=dev)
    mu = torch.empty(batch, dtype=torch.float64, device=dev)
    st = torch.empty(batch, dtype=torch.int32, device=dev)
    nbytes = int(LIB.ace_minl2_workspace_size(batch, m, n, r)) + 256
    ws = (workspace or _DEFAULT_WS).get(nbytes, dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    check(LIB.ace_minl2_admm_batch(C.byref(cfg), batch, m, n, r, int(bool(scale_by_row)), A.data_ptr(), B.data_ptr(),
                                   X0.data_ptr(), ptr(rc), X.data_ptr(), Y.data_ptr(), ptr(Xall), it.data_ptr(),
                                   oc.data_ptr(), obj.data_ptr(), mu.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(),
                                   stream.cuda_stream))
    return MinL2Stage(X, Y, it, oc, obj, mu, st, Xall)


@dataclass
class MinL2Result:
    """The whole recovery.  Without refinement, or after a rollback, Y lives on the train rows (its first m_t entries
    in train order, zeros beyond)."""
    X: object            # [batch][n] complex128
    Y: object            # [batch][m] complex128
    quality: object      # [batch] float64 (NaN without test rows)
    stage_iters: object  # [batch][3] int32: row stage, per-column stage, refinement (0: not run)
    r_used: object       # [batch] int32, the column count of the two r-column stages
    status: object       # [batch] uint32 (host) / int32 (device)
    train_idx: object    # [m_t] int32 (host), the partition used

    @property
    def rolled_back(self):
        return (self.status & ACE_ST_ROLLBACK) != 0


def train_count(m, cc_frac=0.95):
    """m_t = ceil(m cc_frac) (inferMinL2.m:34), as the library computes it."""
    return max(1, min(int(m), math.ceil(m * cc_frac)))


def _partition(train_idx, m, cfg):
    mt = train_count(m, cfg.cc_frac)
    if train_idx is None:
        from .engine import randperm
        return np.ascontiguousarray(randperm(cfg.train_seed, 0, m, mt), dtype=np.int32)
    tr = np.ascontiguousarray(np.asarray(train_idx, dtype=np.int32))
    if tr.shape != (mt,):
        raise ValueError(f"train_idx must be [m_t] = [{mt}] (one partition for the batch), got {tr.shape}")
    return tr


def _solve_cfg(r, maxiter, cc_frac, train_seed, cfg_kw):
    return minl2_cfg(r=int(r), maxiter=int(maxiter), cc_frac=float(cc_frac), train_seed=int(train_seed), **cfg_kw)


def infer_min_l2_host(A, B, train_idx=None, *, r=20, maxiter=500, cc_frac=0.95, train_seed=0, **cfg_kw) -> MinL2Result:
    """inferMinL2 for a batch on host arrays: A [m][n], B [batch][m], ``train_idx`` [m_t] 0-based rows shared by the
    batch (None: drawn from the build's counter RNG with ``train_seed``)."""
    A = np.ascontiguousarray(np.asarray(A, dtype=np.complex128))
    B = np.ascontiguousarray(np.atleast_2d(np.asarray(B, dtype=np.float64)))
    if A.ndim != 2 or B.shape[1] != A.shape[0]:
        raise ValueError(f"A must be [m][n] and B [batch][m], got {A.shape} and {B.shape}")
    m, n = A.shape
    batch = B.shape[0]
    cfg = _solve_cfg(r, maxiter, cc_frac, train_seed, cfg_kw)
    tr = _partition(train_idx, m, cfg)
    X = np.empty((batch, n), np.complex128)
    Y = np.empty((batch, m), np.complex128)
    q = np.empty(batch, np.float64)
    it = np.empty((batch, 3), np.int32)
    ru = np.empty(batch, np.int32)
    st = np.empty(batch, np.uint32)
    dp = lambda a: a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    check(LIB.ace_minl2_solve_host(C.byref(cfg), batch, m, n, dp(A), dp(B), ip(tr), dp(X), dp(Y), dp(q), ip(it), ip(ru),
                                   st.ctypes.data_as(C.POINTER(C.c_uint32))))
    return MinL2Result(X, Y, q, it, ru, st, tr)


def infer_min_l2_batch(A, B, train_idx=None, *, r=20, maxiter=500, cc_frac=0.95, train_seed=0, workspace=None,
                       stream=None, **cfg_kw) -> MinL2Result:
    """inferMinL2 on device tensors: A [m][n] (or [1][m][n]) complex128, B [batch][m] float64; ``train_idx`` is a
    host array.  The call is not asynchronous: the host decides the groups of equal column count and the refinement
    set, so ``stream`` is synchronised at every such round trip (include/ace.h); results stay on the device."""
    import torch
    from .solver import _DEFAULT_WS
    if not (A.is_cuda and B.is_cuda):
        raise ValueError("infer_min_l2_batch needs device tensors")
    if A.dtype != torch.complex128 or B.dtype != torch.float64:
        raise TypeError("A must be complex128 and B float64")
    if A.dim() == 3 and A.shape[0] == 1:
        A = A[0]
    if A.dim() != 2 or B.dim() != 2 or B.shape[1] != A.shape[0] or B.device != A.device:
        raise ValueError(f"A must be [m][n] and B [batch][m] on one device, got {tuple(A.shape)} and {tuple(B.shape)}")
    A, B = A.contiguous(), B.contiguous()
    m, n = A.shape
    batch, dev = B.shape[0], A.device
    cfg = _solve_cfg(r, maxiter, cc_frac, train_seed, cfg_kw)
    tr = _partition(train_idx, m, cfg)
    nbytes = int(LIB.ace_minl2_solve_workspace_size(C.byref(cfg), batch, m, n))
    if nbytes == 0:
        raise ValueError(f"infer_min_l2_batch: sizes outside the limits (batch {batch}, m {m} <= {M_MAX}, n {n} <= {N_MAX})")
    X = torch.empty((batch, n), dtype=torch.complex128, device=dev)
    Y = torch.empty((batch, m), dtype=torch.complex128, device=dev)
    q = torch.empty(batch, dtype=torch.float64, device=dev)
    it = torch.empty((batch, 3), dtype=torch.int32, device=dev)
    ru = torch.empty(batch, dtype=torch.int32, device=dev)
    st = torch.empty(batch, dtype=torch.int32, device=dev)
    ws = (workspace or _DEFAULT_WS).get(nbytes + 256, dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    check(LIB.ace_minl2_solve_batch(C.byref(cfg), batch, m, n, A.data_ptr(), B.data_ptr(),
                                    tr.ctypes.data_as(C.POINTER(C.c_int32)), X.data_ptr(), Y.data_ptr(), q.data_ptr(),
                                    it.data_ptr(), ru.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(),
                                    stream.cuda_stream))
    return MinL2Result(X, Y, q, it, ru, st, tr)


def inferMinL2(A, B, lambda_=0.0, r=20, tol_rel=1e-4, tol_abs=1e-8, maxiter=500, *, train_idx=None, train_seed=0):
    """[X, Y, quality] = inferMinL2(A, B, ...) in the MATLAB calling style, one realisation: X [n][1], Y [m][1]."""
    if lambda_ != 0.0:
        raise ValueError("inferMinL2: only lambda = 0 is implemented (the only value the reference passes)")
    B = np.asarray(B, dtype=np.float64).reshape(1, -1)
    res = infer_min_l2_host(A, B, train_idx, r=r, maxiter=maxiter, train_seed=train_seed, tol_rel=tol_rel, tol_abs=tol_abs)
    return res.X[0].reshape(-1, 1), res.Y[0].reshape(-1, 1), float(res.quality[0])
