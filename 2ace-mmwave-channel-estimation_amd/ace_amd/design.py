"""Bayesian A-optimal probe selection on the GPU (``ace_aopt_select_*``, csrc/ace_aopt.hip): which M probes of a
codebook to measure.  The reference's ``Bayes_Beam.m`` -> ``bayesAopt_complex.m`` (the ``'Bayes_Beam'`` mode of
``Generate_Sensing_Matrix_with_candidate.m``): a Fedorov row exchange that picks rows X of a candidate codebook F to
minimise trace((X^H X + kdiag I)^-1), the posterior variance of the channel estimate, with A = I and no fixed rows.

Passes over the design's rows repeat while some row switched and ``iter < maxiter``.  For each row the exchange value
``ad_i`` of replacing it by candidate i is formed for every candidate (one product of F with two vectors, on the f64
matrix cores); the row switches to the first index of the minimum when that minimum is below ``acutoff = -sqrt(eps)``
or the row is still unassigned.  include/ace.h and csrc/ace_aopt.hip state the step.  Designs of one call share F and
run side by side; a design's result does not depend on the others.

Entry points (no CPU fallback -- every call runs the kernels on the GPU):
  * ``aopt_select_batch(F, nrows, init)`` -- device tensors in, device tensors out.
  * ``aopt_select_host(F, nrows, init)`` -- numpy arrays.
  * ``bayes_beam(cb, M, seed=...)`` -- the ``Bayes_Beam.m`` call: M rows of ``cb``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import LIB, check, aopt_cfg, ACE_ST_AOPT_SINGULAR
from . import synth

N_MAX, P_MAX, ROWS_MAX = 1024, 65536, 4096   # the C-ABI's limits (include/ace.h)
ST_AOPT = 9                                   # stream kind of the start rows (synth.stream_id)


@dataclass
class AoptResult:
    rowlist: object    # [designs][nrows_max] int32: the candidate of every design row, -1 past nrows[d]
    acrit: object      # [designs][2] float64: trace of the start's inverse, tracked trace at the end
    iters: object      # [designs] int32 passes run
    switches: object   # [designs] int32 rows switched
    status: object     # [designs] uint32 (host) / int32 (device): ACE_ST_AOPT_SINGULAR
    Minv: object = None   # [designs][n][n] complex128 tracked (X^H X + kdiag I)^-1, or None when not requested

    @property
    def singular(self):
        return (self.status & ACE_ST_AOPT_SINGULAR) != 0


def _shapes(fs, nrows, init_shape):
    """(designs, P, n, nrows_max) of F [P][n], nrows [designs], init [designs][nrows_max]."""
    if len(fs) != 2 or not 1 <= fs[0] <= P_MAX or not 1 <= fs[1] <= N_MAX:
        raise ValueError(f"F must be [P][n] with 1 <= P <= {P_MAX} and 1 <= n <= {N_MAX}, got {tuple(fs)}")
    if len(init_shape) != 2 or init_shape[0] < 1 or not 1 <= init_shape[1] <= ROWS_MAX:
        raise ValueError(f"init must be [designs][nrows_max] with 1 <= nrows_max <= {ROWS_MAX}, got {tuple(init_shape)}")
    if tuple(nrows) != (init_shape[0],):
        raise ValueError(f"nrows must be [designs] = [{init_shape[0]}], got {tuple(nrows)}")
    return init_shape[0], fs[0], fs[1], init_shape[1]


def _cfg(kdiag, maxiter):
    return aopt_cfg(kdiag=float(kdiag), maxiter=int(maxiter))


def aopt_select_host(F, nrows, init, *, kdiag=1.0, maxiter=5, want_minv=False) -> AoptResult:
    """The row exchange on host arrays: F [P][n] complex, nrows [designs] (or one int), init [designs][nrows_max]
    (or [nrows]) start candidates, read up to nrows[d] per design."""
    F = np.ascontiguousarray(np.atleast_2d(np.asarray(F, dtype=np.complex128)))
    init = np.ascontiguousarray(np.atleast_2d(np.asarray(init, dtype=np.int32)))
    nrows = np.ascontiguousarray(np.asarray(nrows, dtype=np.int32).reshape(-1))
    designs, P, n, rmax = _shapes(F.shape, nrows.shape, init.shape)
    rowlist = np.empty((designs, rmax), np.int32)
    acrit = np.empty((designs, 2), np.float64)
    iters = np.empty(designs, np.int32)
    sw = np.empty(designs, np.int32)
    st = np.empty(designs, np.uint32)
    Minv = np.empty((designs, n, n), np.complex128) if want_minv else None
    dp = lambda a: None if a is None else a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    cfg = _cfg(kdiag, maxiter)
    check(LIB.ace_aopt_select_host(C.byref(cfg), designs, P, n, rmax, dp(F), ip(nrows), ip(init), ip(rowlist), dp(acrit),
                                   ip(iters), ip(sw), st.ctypes.data_as(C.POINTER(C.c_uint32)), dp(Minv)))
    return AoptResult(rowlist, acrit, iters, sw, st, Minv)


def aopt_select_batch(F, nrows, init, *, kdiag=1.0, maxiter=5, want_minv=False, workspace=None, stream=None) -> AoptResult:
    """The row exchange on device tensors: F [P][n] complex128, nrows [designs] int32, init [designs][nrows_max] int32
    (start candidates, read up to nrows[d]; entries outside 0..P-1 are clamped).  Enqueued on ``stream`` (default: the
    current stream), which is synchronised once per pass.  ``workspace``: a ``solver.Workspace`` (default: the
    package's shared one)."""
    import torch
    from .solver import _DEFAULT_WS
    if not all(t.is_cuda for t in (F, nrows, init)):
        raise ValueError("aopt_select_batch needs device tensors")
    if F.dtype != torch.complex128:
        raise TypeError("F must be complex128")
    if nrows.dtype != torch.int32 or init.dtype != torch.int32:
        raise TypeError("nrows and init must be int32")
    designs, P, n, rmax = _shapes(tuple(F.shape), tuple(nrows.shape), tuple(init.shape))
    dev = F.device
    if nrows.device != dev or init.device != dev:
        raise ValueError("F, nrows and init must be on one device")
    F, nrows, init = F.contiguous(), nrows.contiguous(), init.contiguous()
    rowlist = torch.empty((designs, rmax), dtype=torch.int32, device=dev)
    acrit = torch.empty((designs, 2), dtype=torch.float64, device=dev)
    iters = torch.empty(designs, dtype=torch.int32, device=dev)
    sw = torch.empty(designs, dtype=torch.int32, device=dev)
    st = torch.empty(designs, dtype=torch.int32, device=dev)
    Minv = torch.empty((designs, n, n), dtype=torch.complex128, device=dev) if want_minv else None
    nbytes = int(LIB.ace_aopt_workspace_size(designs, P, n, rmax)) + 256
    ws = (workspace or _DEFAULT_WS).get(nbytes, dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    cfg = _cfg(kdiag, maxiter)
    check(LIB.ace_aopt_select_batch(C.byref(cfg), designs, P, n, rmax, F.data_ptr(), nrows.data_ptr(), init.data_ptr(),
                                    rowlist.data_ptr(), acrit.data_ptr(), iters.data_ptr(), sw.data_ptr(), st.data_ptr(),
                                    None if Minv is None else Minv.data_ptr(), ws.data_ptr(), ws.numel(),
                                    stream.cuda_stream))
    return AoptResult(rowlist, acrit, iters, sw, st, Minv)


def start_rows(seed, stream_id, P, M):
    """M start candidates in 0..P-1, drawn with replacement (bayesAopt_complex.m:128, unidrnd) from the build's
    counter generator: floor(P u01(seed, stream_id(ST_AOPT, stream_id), r)), r = 0 .. M-1."""
    u = synth.u01(seed, synth.stream_id(ST_AOPT, int(stream_id)), np.arange(int(M), dtype=np.uint64))
    return np.minimum((u * int(P)).astype(np.int64), int(P) - 1).astype(np.int32)


def bayes_beam(cb, M, *, seed, stream_id=0, candidates=None, kdiag=1.0, maxiter=5, device=None):
    """``Bayes_Beam(M, ULA, cb_train, num_sel)``: M rows of the codebook ``cb`` [P][n] (numpy or tensor) chosen by the
    row exchange with K = I.  Returns the picked rows as int64 indices into ``cb`` ([M], in design-row order; a row may
    be picked more than once, as in the reference).

    ``candidates``: indices into ``cb`` that form the candidate set (default: every row).  Departure from the
    reference: Bayes_Beam.m draws 40000 candidates with replacement from the pool (``randi(num_sel, 40000, 1)``),
    which is the pool with multiplicities; a duplicate never changes an exchange value and ties go to the first
    index, so the candidate set here is the pool itself, each row once.  The start rows come from the build's
    counter generator (``start_rows``; MATLAB's unidrnd stream cannot be reproduced), drawn with replacement as the
    reference does.  A design the kernels stop (ACE_ST_AOPT_SINGULAR) raises."""
    import torch
    dev = torch.device("cuda" if device is None else device)
    host = lambda a: np.array(a) if isinstance(a, np.ndarray) else a   # noqa: E731  (a copy: the input may be read-only)
    cb = torch.as_tensor(host(cb), device=dev).to(torch.complex128)
    if cb.dim() != 2:
        raise ValueError(f"cb must be [P][n], got {tuple(cb.shape)}")
    cand = np.arange(cb.shape[0], dtype=np.int64) if candidates is None else np.asarray(candidates, np.int64).reshape(-1)
    if cand.size < 1 or cand.min() < 0 or cand.max() >= cb.shape[0]:
        raise ValueError(f"candidates must be indices in 0..{cb.shape[0] - 1}")
    M = int(M)
    if not 1 <= M <= ROWS_MAX:
        raise ValueError(f"M must be in 1..{ROWS_MAX}, got {M}")
    F = cb if candidates is None else cb[torch.as_tensor(cand, device=dev)]
    init = torch.as_tensor(start_rows(seed, stream_id, cand.size, M)[None], device=dev)
    nrows = torch.full((1,), M, dtype=torch.int32, device=dev)
    res = aopt_select_batch(F.contiguous(), nrows, init, kdiag=kdiag, maxiter=maxiter)
    if int(res.status[0].item()) & ACE_ST_AOPT_SINGULAR:
        raise RuntimeError("bayes_beam: the row exchange met a singular removal (ACE_ST_AOPT_SINGULAR)")
    return cand[res.rowlist[0].cpu().numpy().astype(np.int64)]
