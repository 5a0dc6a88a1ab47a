"""Batched PR-GAMP on the GPU (``ace_prgamp_solve_*``, csrc/ace_prgamp.hip): the PRGAMP baseline of the reference's
Vs_M.m (MyCPR.m:110-120 -> MyPRGAMP.m:71 -> prGAMP4), compressive phase retrieval straight from the magnitude
measurements, without the PhaseLift compression stage the two-stage recoveries are argued against it with.

The reference vendors the solver under ``3rd_software_component/GAMP/trunk/code`` (``phase/prGAMP4.m``,
``phase/ncCAwgnEstimOut.m``, ``main/gampEst.m``, ``main/estimInvert.m``, ``main/CAwgnEstimIn.m``,
``main/SparseScaEstim.m``, ``main/GampOpt.m``); the kernel restates it for the option set of MyCPR.m, one column per
realisation, against one shared matrix ``D`` [m][N]: message passing under the non-coherent output channel with the
Bethe cost for the adaptive step, an EM loop that learns the noise variance and tunes the Bernoulli-Gaussian prior, and
random restarts.  include/ace.h and the kernel's header state the iteration and the reference's quirks it keeps.

Random restarts: MATLAB's ``randn`` stream cannot be reproduced, so the draws are an input, ``draws`` [batch][max_try][N]
complex with real and imaginary parts of unit variance (``randn(nx, 2) * [1; 1i]`` of prGAMP4.m:608).  ``draws=None``
generates them from ``seed`` with the package's counter generator (``synth.sm64``), not torch's global state:
realisation b, try t, atom j takes the Box-Muller pair of counters 2 c and 2 c + 1, c = t N + j, of stream
``synth.stream_id(ST_PRGAMP, b)`` -- on the host ``synth.normal_pairs(seed, synth.stream_id(ST_PRGAMP, b), max_try * N)``
reshaped to [max_try][N] (``prgamp_draws_host``; the integer streams are identical, the floating-point Box-Muller
step agrees to the rounding of log / cos / sin).  They cost 16 batch max_try N bytes.

A realisation with a non-finite ``abs_y`` returns zeros and ACE_ST_EVAL_DEGENERATE; where the reference would raise
(MyPRGAMP's catch returns zeros) it returns zeros and ACE_ST_PRGAMP_FAILED; when the tries run out above the stop
level it returns the best try and ACE_ST_PRGAMP_MAXTRY, as the reference does.

Entry points (no CPU fallback -- every call runs ``prgamp_kernel`` on the GPU):
  * ``prgamp_host(D, abs_y, s_over_n, ...)``  -- numpy arrays.
  * ``prgamp_batch(D, abs_y, s_over_n, ...)`` -- device tensors already in HBM; no host copy.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import synth
from ._lib import LIB, check, prgamp_cfg, ACE_ST_EVAL_DEGENERATE, ACE_ST_PRGAMP_FAILED, ACE_ST_PRGAMP_MAXTRY

M_MAX, N_MAX = 256, 16384   # the C-ABI's limits (include/ace.h)
ST_PRGAMP = 7               # stream kind of the restart draws (synth.stream_id)


@dataclass
class PrGampResult:
    xhat: object       # [batch][N] complex128, the best try's estimate (defined up to a global phase)
    info: object       # [batch][8] float64: best residual dB, wvar, sparseRat_hat, xvar0_hat, xmean0sq_hat, SNRdB_est, 0, 0
    counts: object     # [batch][4] int32: numTry, best try (1-based), EM iterations of the best try, support_size (-1: NaN)
    status: object     # [batch] uint32 (host) / int32 (device)
    trace: object = None   # [batch][max_try][nit_em + 1][2] int32 (iterations, passed iterations) per GAMP call, or None
    vals: object = None    # [batch][max_try][nit_em + 1] float64, the last passed utility of each call, or None

    @property
    def failed(self):
        return (self.status & ACE_ST_PRGAMP_FAILED) != 0

    @property
    def degenerate(self):
        return (self.status & ACE_ST_EVAL_DEGENERATE) != 0

    @property
    def max_try(self):
        return (self.status & ACE_ST_PRGAMP_MAXTRY) != 0

    @property
    def tries(self):
        return self.counts[:, 0]

    def channel(self, AD):
        """``AD @ xhat`` per realisation ([batch][rows of AD]), as ``OmpResult.channel``."""
        if isinstance(self.xhat, np.ndarray):
            return self.xhat @ np.asarray(AD).T
        return (self.xhat @ AD.transpose(0, 1)).contiguous()


def _s64(c):
    c &= (1 << 64) - 1
    return c - (1 << 64) if c >= (1 << 63) else c


def prgamp_draws(seed, batch, max_try, N, device, first=0):
    """The restart draws [batch][max_try][N] complex128 on ``device`` from the counter generator (module text);
    ``first``: the index of the first realisation (its stream is that of realisation first + b)."""
    import torch
    i64 = dict(dtype=torch.int64, device=device)

    def lsr(z, k):
        return (z >> k) & ((1 << (64 - k)) - 1)

    stream = ST_PRGAMP + 16 * (torch.arange(batch, **i64) + (int(first) + 1))
    base = (stream * _s64(int(synth._C1))) ^ _s64(int(seed))
    c = torch.arange(max_try * N, **i64)

    def u01(ctr):
        z = base[:, None] + (ctr[None, :] + 1) * _s64(int(synth._C2))
        z = (z ^ lsr(z, 30)) * _s64(int(synth._M1))
        z = (z ^ lsr(z, 27)) * _s64(int(synth._M2))
        z = z ^ lsr(z, 31)
        return lsr(z, 11).to(torch.float64) * (1.0 / 9007199254740992.0)

    u1, u2 = u01(2 * c), u01(2 * c + 1)
    r = torch.sqrt(-2.0 * torch.log(1.0 - u1))
    g = torch.complex(r * torch.cos(2.0 * np.pi * u2), r * torch.sin(2.0 * np.pi * u2))
    return g.reshape(batch, max_try, N)


def prgamp_draws_host(seed, batch, max_try, N, first=0):
    """The host twin of ``prgamp_draws`` (numpy)."""
    return np.stack([synth.normal_pairs(seed, synth.stream_id(ST_PRGAMP, int(first) + b), max_try * N).reshape(max_try, N)
                     for b in range(batch)])


def _shapes(ds, ys):
    if len(ds) != 2 or not 1 <= ds[0] <= M_MAX or not 1 <= ds[1] <= N_MAX:
        raise ValueError(f"D must be [m][N] with 1 <= m <= {M_MAX} and 1 <= N <= {N_MAX}, got {tuple(ds)}")
    m, N = ds
    if len(ys) != 2 or ys[0] < 1 or ys[1] != m:
        raise ValueError(f"abs_y must be [batch][m] = [batch][{m}], got {tuple(ys)}")
    return ys[0], m, N


def prgamp_host(D, abs_y, s_over_n, *, draws=None, seed=None, max_try=100, nit_em=50, gamp_nit=200, trace=False,
                **cfg_kw) -> PrGampResult:
    """PR-GAMP for a batch on host arrays (see the module text).  ``cfg_kw``: snr_db, snr_db_init."""
    D = np.ascontiguousarray(np.atleast_2d(np.asarray(D, dtype=np.complex128)))
    Y = np.ascontiguousarray(np.atleast_2d(np.asarray(abs_y, dtype=np.float64)))
    batch, m, N = _shapes(D.shape, Y.shape)
    cfg = prgamp_cfg(sparse_rat=float(s_over_n), max_try=int(max_try), nit_em=int(nit_em), gamp_nit=int(gamp_nit), **cfg_kw)
    if draws is None:
        if seed is None:
            raise ValueError("prgamp_host needs draws or a seed")
        draws = prgamp_draws_host(seed, batch, cfg.max_try, N)
    G = np.ascontiguousarray(np.asarray(draws, dtype=np.complex128))
    if G.shape != (batch, cfg.max_try, N):
        raise ValueError(f"draws must be [batch][max_try][N] = {(batch, cfg.max_try, N)}, got {G.shape}")
    xhat = np.empty((batch, N), np.complex128)
    info = np.empty((batch, 8), np.float64)
    cnt = np.empty((batch, 4), np.int32)
    st = np.empty(batch, np.uint32)
    tr = np.empty((batch, cfg.max_try, cfg.nit_em + 1, 2), np.int32) if trace else None
    vals = np.empty((batch, cfg.max_try, cfg.nit_em + 1), np.float64) if trace else None
    dp = lambda a: None if a is None else a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    check(LIB.ace_prgamp_solve_host(C.byref(cfg), batch, m, N, dp(D), dp(Y), dp(G), dp(xhat), dp(info), ip(cnt),
                                    st.ctypes.data_as(C.POINTER(C.c_uint32)), ip(tr), dp(vals)))
    return PrGampResult(xhat, info, cnt, st, tr, vals)


def prgamp_batch(D, abs_y, s_over_n, *, draws=None, seed=None, max_try=100, nit_em=50, gamp_nit=200, trace=False,
                 first=0, workspace=None, stream=None, **cfg_kw) -> PrGampResult:
    """PR-GAMP on device tensors: D [m][N] complex128, abs_y [batch][m] float64 (the magnitudes), ``s_over_n`` the
    sparsity rate handed to the prior (s / n in MyCPR.m).  ``draws`` [batch][max_try][N] complex128 on the device, or
    ``seed`` to generate them there (``first``: the stream index of realisation 0).  ``trace=True`` also returns the
    per-call iteration counts and utilities.  Asynchronous on ``stream`` (default: the current stream); nothing is
    copied to the host.  ``workspace``: a ``solver.Workspace`` to take the state vectors from (default: the package's
    shared one).  ``cfg_kw``: snr_db (25), snr_db_init (20)."""
    import torch
    from .solver import _DEFAULT_WS
    if not (D.is_cuda and abs_y.is_cuda):
        raise ValueError("prgamp_batch needs device tensors")
    if D.dtype != torch.complex128 or abs_y.dtype != torch.float64:
        raise TypeError("D must be complex128 and abs_y float64")
    batch, m, N = _shapes(tuple(D.shape), tuple(abs_y.shape))
    dev = D.device
    if abs_y.device != dev:
        raise ValueError("D and abs_y must be on one device")
    cfg = prgamp_cfg(sparse_rat=float(s_over_n), max_try=int(max_try), nit_em=int(nit_em), gamp_nit=int(gamp_nit), **cfg_kw)
    if draws is None:
        if seed is None:
            raise ValueError("prgamp_batch needs draws or a seed")
        draws = prgamp_draws(seed, batch, cfg.max_try, N, dev, first=first)
    if draws.dtype != torch.complex128 or tuple(draws.shape) != (batch, cfg.max_try, N) or draws.device != dev:
        raise ValueError(f"draws must be complex128 [batch][max_try][N] = {(batch, cfg.max_try, N)} on {dev}")
    D, Y, G = D.contiguous(), abs_y.contiguous(), draws.contiguous()
    xhat = torch.empty((batch, N), dtype=torch.complex128, device=dev)
    info = torch.empty((batch, 8), dtype=torch.float64, device=dev)
    cnt = torch.empty((batch, 4), dtype=torch.int32, device=dev)
    st = torch.empty(batch, dtype=torch.int32, device=dev)
    tr = torch.empty((batch, cfg.max_try, cfg.nit_em + 1, 2), dtype=torch.int32, device=dev) if trace else None
    vals = torch.empty((batch, cfg.max_try, cfg.nit_em + 1), dtype=torch.float64, device=dev) if trace else None
    nbytes = int(LIB.ace_prgamp_workspace_size(batch, m, N, cfg.max_try)) + 256
    ws = (workspace or _DEFAULT_WS).get(nbytes, dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    check(LIB.ace_prgamp_solve_batch(C.byref(cfg), batch, m, N, D.data_ptr(), Y.data_ptr(), G.data_ptr(), xhat.data_ptr(),
                                     info.data_ptr(), cnt.data_ptr(), st.data_ptr(), ptr(tr), ptr(vals), ws.data_ptr(),
                                     ws.numel(), stream.cuda_stream))
    return PrGampResult(xhat, info, cnt, st, tr, vals)
