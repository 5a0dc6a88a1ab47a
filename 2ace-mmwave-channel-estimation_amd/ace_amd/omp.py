"""Batched orthogonal matching pursuit on the GPU (``ace_omp_solve_*``, csrc/ace_omp.hip): the sparse solver of the
two-stage PLOMP recovery and of the coherent-measurement benchmark (``sparse.py``).  Per realisation, against one
shared dictionary ``D`` [d][N]::

    r = y, I = {}
    repeat: stop if |I| = kmax or ||r||_2 <= tol
            j = argmax over j not in I of w_j |d_j^H r|^2        (ties: smaller j; w = colscale or 1)
            I <- I u {j};  c = argmin ||y - D_I c||_2;  r = y - D_I c

The reference calls ``OMP(C, intSoln, 1e-12)`` and ``OMP(A, y, s)``; ``OMP.m`` itself comes from the external
CoSaMP_OMP toolbox and is not in the reference tree.  This is textbook OMP with both stopping rules (an atom count
and an absolute residual-norm tolerance); reading a third argument below 1 as a tolerance is this project's
interpretation of the call sites, not a transcription.

A realisation with a non-finite ``y`` returns count 0, indices -1 and ACE_ST_EVAL_DEGENERATE; ``y = 0`` (or
``||y|| <= tol``) count 0 and no flag; an atom that is numerically dependent on the chosen ones is not added, and
the realisation stops with ACE_ST_OMP_DEPENDENT (include/ace.h states the test).

Entry points (no CPU fallback -- every call runs ``omp_kernel`` on the GPU):
  * ``omp_host(D, Y, kmax, tol)`` -- numpy arrays.
  * ``omp_batch(D, Y, kmax, tol)`` -- device tensors already in HBM; no host copy.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import LIB, check, ACE_ST_EVAL_DEGENERATE, ACE_ST_OMP_DEPENDENT

D_MAX, N_MAX = 256, 16384   # the C-ABI's limits (include/ace.h)


@dataclass
class OmpResult:
    idx: object       # [batch][kmax] int32, selection order, -1 past count
    coef: object      # [batch][kmax] complex128, same order, 0 past count
    count: object     # [batch] int32
    resnorm: object   # [batch] float64, the final ||r||_2
    status: object    # [batch] uint32 (host) / int32 (device): ACE_ST_EVAL_DEGENERATE, ACE_ST_OMP_DEPENDENT
    N: int
    x: object = None  # [batch][N] complex128 dense solution, or None when not requested

    @property
    def degenerate(self):
        return (self.status & ACE_ST_EVAL_DEGENERATE) != 0

    @property
    def dependent(self):
        return (self.status & ACE_ST_OMP_DEPENDENT) != 0

    def channel(self, AD):
        """``AD[:, idx] @ coef`` per realisation ([batch][rows of AD]): the signal the support and its
        coefficients stand for in the column space of ``AD`` [rows][N] (Recover_Channel.m: AD * plomp_signal)."""
        if isinstance(self.idx, np.ndarray):
            G = np.asarray(AD)[:, np.maximum(self.idx, 0).astype(np.int64)]       # [rows][batch][kmax]
            return np.einsum("rbk,bk->br", G, self.coef)                          # (coef is 0 past count)
        G = AD[:, self.idx.clamp(min=0).long()]
        return (G * self.coef.unsqueeze(0)).sum(dim=2).transpose(0, 1).contiguous()


def _shapes(ds, ys, ws, kmax):
    """(batch, d, N) of D [d][N], Y [batch][d], colscale None or [N]."""
    if len(ds) != 2 or not 1 <= ds[0] <= D_MAX or not 1 <= ds[1] <= N_MAX:
        raise ValueError(f"D must be [d][N] with 1 <= d <= {D_MAX} and 1 <= N <= {N_MAX}, got {tuple(ds)}")
    d, N = ds
    if len(ys) != 2 or ys[0] < 1 or ys[1] != d:
        raise ValueError(f"Y must be [batch][d] = [batch][{d}], got {tuple(ys)}")
    if ws is not None and tuple(ws) != (N,):
        raise ValueError(f"colscale must be [N] = [{N}], got {tuple(ws)}")
    if not 1 <= kmax <= min(d, N):
        raise ValueError(f"kmax must be in 1..min(d = {d}, N = {N}), got {kmax}")
    return ys[0], d, N


def omp_host(D, Y, kmax, tol=0.0, colscale=None, want_x=False) -> OmpResult:
    """OMP for a batch on host arrays (see the module text)."""
    D = np.ascontiguousarray(np.atleast_2d(np.asarray(D, dtype=np.complex128)))
    Y = np.ascontiguousarray(np.atleast_2d(np.asarray(Y, dtype=np.complex128)))
    if colscale is not None:
        colscale = np.ascontiguousarray(np.asarray(colscale, dtype=np.float64))
    kmax, tol = int(kmax), float(tol)
    batch, d, N = _shapes(D.shape, Y.shape, None if colscale is None else colscale.shape, kmax)
    idx = np.empty((batch, kmax), np.int32)
    coef = np.empty((batch, kmax), np.complex128)
    cnt = np.empty(batch, np.int32)
    rn = np.empty(batch, np.float64)
    st = np.empty(batch, np.uint32)
    x = np.empty((batch, N), np.complex128) if want_x else None
    dp = lambda a: None if a is None else a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    check(LIB.ace_omp_solve_host(batch, d, N, kmax, tol, dp(D), dp(colscale), dp(Y), ip(idx), dp(coef), ip(cnt), dp(rn),
                                 st.ctypes.data_as(C.POINTER(C.c_uint32)), dp(x)))
    return OmpResult(idx, coef, cnt, rn, st, N, x)


def omp_batch(D, Y, kmax, tol=0.0, colscale=None, want_x=False, *, workspace=None, stream=None) -> OmpResult:
    """OMP on device tensors: D [d][N] and Y [batch][d] complex128, colscale None or [N] float64.  Asynchronous
    on ``stream`` (default: the current stream); nothing is copied to the host.  ``workspace``: a
    ``solver.Workspace`` to take the QR factors from (default: the package's shared one)."""
    import torch
    from .solver import _DEFAULT_WS
    ts = [D, Y] + ([] if colscale is None else [colscale])
    if not all(t.is_cuda for t in ts):
        raise ValueError("omp_batch needs device tensors")
    if D.dtype != torch.complex128 or Y.dtype != torch.complex128:
        raise TypeError("D and Y must be complex128")
    if colscale is not None and colscale.dtype != torch.float64:
        raise TypeError("colscale must be float64")
    kmax, tol = int(kmax), float(tol)
    batch, d, N = _shapes(tuple(D.shape), tuple(Y.shape), None if colscale is None else tuple(colscale.shape), kmax)
    dev = D.device
    if any(t.device != dev for t in ts):
        raise ValueError("D, Y and colscale must be on one device")
    D, Y = D.contiguous(), Y.contiguous()
    if colscale is not None:
        colscale = colscale.contiguous()
    idx = torch.empty((batch, kmax), dtype=torch.int32, device=dev)
    coef = torch.empty((batch, kmax), dtype=torch.complex128, device=dev)
    cnt = torch.empty(batch, dtype=torch.int32, device=dev)
    rn = torch.empty(batch, dtype=torch.float64, device=dev)
    st = torch.empty(batch, dtype=torch.int32, device=dev)
    x = torch.empty((batch, N), dtype=torch.complex128, device=dev) if want_x else None
    nbytes = int(LIB.ace_omp_workspace_size(batch, d, N, kmax)) + 256
    ws = (workspace or _DEFAULT_WS).get(nbytes, dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    check(LIB.ace_omp_solve_batch(batch, d, N, kmax, tol, D.data_ptr(), ptr(colscale), Y.data_ptr(), idx.data_ptr(),
                                  coef.data_ptr(), cnt.data_ptr(), rn.data_ptr(), st.data_ptr(), ptr(x), ws.data_ptr(),
                                  ws.numel(), stream.cuda_stream))
    return OmpResult(idx, coef, cnt, rn, st, N, x)
