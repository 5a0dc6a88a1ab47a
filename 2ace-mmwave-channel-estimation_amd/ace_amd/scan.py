"""Beam scan on the GPU: the reference's exhaustive sweep (MyBeamSweeping.m:93-125) and the angular map
``Leakage = A_Rx' * H * A_Tx`` (Sparse_Channel_Formulation.m:149), batched and fused with the selection::

    y[b][p][q] = sum_i sum_j conj(W0[q][i]) x_b[i + d0 j] F1[p][j]        (w' * H * f)
    P          = |y + noise|^2,   flat index f = p Q0 + q                  (:124-125, zero-based)

``X`` [batch][d0*d1] holds mat(x)(i, j) = x[i + d0 j] (the layout ``evaluate_batch`` takes), ``W0`` [Q0][d0] the
beams on the leading index (applied conjugated), ``F1`` [Q1][d1] those on the trailing index (applied plain);
with the synth's vec(H) order the leading index is the receive antenna, so W0 holds combiners and F1 precoders.
Per realisation the K largest P come back in descending order, equal powers by increasing f.  A realisation
whose x, or whose noise row, holds a non-finite value returns powers 0, indices -1, total 0 and
ACE_ST_EVAL_DEGENERATE; an all-zero x is not degenerate.

Entry points (no CPU fallback -- every call runs ``scan_kernel`` on the GPU):
  * ``beam_scan_host(X, W0, F1, K)`` -- numpy arrays.
  * ``beam_scan_batch(X, W0, F1, K)`` -- device tensors already in HBM; no host copy.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import LIB, check, ACE_ST_EVAL_DEGENERATE

K_MAX, D_MAX, Q_MAX = 16, 32, 4096   # the C-ABI's limits (include/ace.h)


@dataclass
class ScanResult:
    top_pow: object   # [batch][K] float64, descending
    top_idx: object   # [batch][K] int32, f = p Q0 + q (-1: degenerate realisation)
    Q0: int
    status: object    # [batch] uint32 (host) / int32 (device): ACE_ST_EVAL_DEGENERATE
    total: object = None   # [batch] float64 sum of P, or None when not requested
    power: object = None   # [batch][Q1][Q0] float64, or None when not requested

    @property
    def p(self):
        """Index into F1 of each entry (ind_F - 1); -1 where top_idx is -1."""
        return self.top_idx // self.Q0 if _is_np(self.top_idx) else self.top_idx.div(self.Q0, rounding_mode="floor")

    @property
    def q(self):
        """Index into W0 of each entry (ind_W - 1); -1 where top_idx is -1."""
        return self.top_idx - self.p * self.Q0 + (self.top_idx < 0) * (-self.Q0)

    @property
    def degenerate(self):
        return (self.status & ACE_ST_EVAL_DEGENERATE) != 0


def _is_np(a):
    return isinstance(a, np.ndarray)


def _shapes(xs, ws, fs, ns, K):
    """(batch, d0, d1, Q0, Q1) of X [batch][d0*d1], W0 [Q0][d0], F1 [Q1][d1], noise None or [batch][Q1*Q0]."""
    if len(ws) != 2 or len(fs) != 2 or ws[0] < 1 or fs[0] < 1 or not 1 <= ws[1] <= D_MAX or not 1 <= fs[1] <= D_MAX:
        raise ValueError(f"W0 must be [Q0][d0] and F1 [Q1][d1] with 1 <= d0, d1 <= {D_MAX}, got {tuple(ws)} and {tuple(fs)}")
    (Q0, d0), (Q1, d1) = ws, fs
    if Q0 > Q_MAX or Q1 > Q_MAX:
        raise ValueError(f"at most {Q_MAX} beams per side, got Q0 = {Q0}, Q1 = {Q1}")
    if len(xs) != 2 or xs[0] < 1 or xs[1] != d0 * d1:
        raise ValueError(f"X must be [batch][d0*d1] = [batch][{d0 * d1}], got {tuple(xs)}")
    if ns is not None and tuple(ns) not in ((xs[0], Q1 * Q0), (xs[0], Q1, Q0)):
        raise ValueError(f"noise must be [batch][Q1*Q0] = [{xs[0]}][{Q1 * Q0}], got {tuple(ns)}")
    if not 1 <= K <= min(K_MAX, Q0 * Q1):
        raise ValueError(f"K must be in 1..min({K_MAX}, Q0*Q1 = {Q0 * Q1}), got {K}")
    return xs[0], d0, d1, Q0, Q1


def beam_scan_host(X, W0, F1, K=1, noise=None, want_power=False, want_total=False) -> ScanResult:
    """The beam scan for a batch on host arrays (complex; see the module text for the layouts)."""
    X = np.ascontiguousarray(np.atleast_2d(np.asarray(X, dtype=np.complex128)))
    W0 = np.ascontiguousarray(np.atleast_2d(np.asarray(W0, dtype=np.complex128)))
    F1 = np.ascontiguousarray(np.atleast_2d(np.asarray(F1, dtype=np.complex128)))
    if noise is not None:
        noise = np.ascontiguousarray(np.asarray(noise, dtype=np.complex128))
    K = int(K)
    batch, d0, d1, Q0, Q1 = _shapes(X.shape, W0.shape, F1.shape, None if noise is None else noise.shape, K)
    tp = np.empty((batch, K), np.float64)
    ti = np.empty((batch, K), np.int32)
    st = np.empty(batch, np.uint32)
    tot = np.empty(batch, np.float64) if want_total else None
    pw = np.empty((batch, Q1, Q0), np.float64) if want_power else None
    dp = lambda a: None if a is None else a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    check(LIB.ace_beam_scan_host(batch, d0, d1, Q0, Q1, dp(X), dp(W0), dp(F1), dp(noise), K, dp(tp),
                                 ti.ctypes.data_as(C.POINTER(C.c_int32)), dp(tot), dp(pw),
                                 st.ctypes.data_as(C.POINTER(C.c_uint32))))
    return ScanResult(tp, ti, Q0, st, tot, pw)


def beam_scan_batch(X, W0, F1, K=1, noise=None, want_power=False, want_total=False, *, stream=None) -> ScanResult:
    """The beam scan on device tensors: X [batch][d0*d1], W0 [Q0][d0], F1 [Q1][d1], noise None or
    [batch][Q1*Q0], all complex128.  Asynchronous on ``stream`` (default: the current stream); nothing is
    copied to the host."""
    import torch
    ts = [X, W0, F1] + ([] if noise is None else [noise])
    if not all(t.is_cuda for t in ts):
        raise ValueError("beam_scan_batch needs device tensors")
    if any(t.dtype != torch.complex128 for t in ts):
        raise TypeError("X, W0, F1 and noise must be complex128")
    K = int(K)
    batch, d0, d1, Q0, Q1 = _shapes(tuple(X.shape), tuple(W0.shape), tuple(F1.shape),
                                    None if noise is None else tuple(noise.shape), K)
    dev = X.device
    if any(t.device != dev for t in ts):
        raise ValueError("X, W0, F1 and noise must be on one device")
    X, W0, F1 = X.contiguous(), W0.contiguous(), F1.contiguous()
    if noise is not None:
        noise = noise.contiguous()
    tp = torch.empty((batch, K), dtype=torch.float64, device=dev)
    ti = torch.empty((batch, K), dtype=torch.int32, device=dev)
    st = torch.empty(batch, dtype=torch.int32, device=dev)
    tot = torch.empty(batch, dtype=torch.float64, device=dev) if want_total else None
    pw = torch.empty((batch, Q1, Q0), dtype=torch.float64, device=dev) if want_power else None
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    check(LIB.ace_beam_scan_batch(batch, d0, d1, Q0, Q1, X.data_ptr(), W0.data_ptr(), F1.data_ptr(), ptr(noise), K,
                                  tp.data_ptr(), ti.data_ptr(), ptr(tot), ptr(pw), st.data_ptr(), stream.cuda_stream))
    return ScanResult(tp, ti, Q0, st, tot, pw)
