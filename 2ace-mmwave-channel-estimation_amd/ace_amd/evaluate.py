"""Channel evaluation on the GPU: the reference's ``Evaluation_H``
(Numerical_Simulation/src/evaluate_plot_results/Evaluation_H.m:73-132), batched.

Per realisation, from the estimate x and the truth g (vec(H) order, n = tx*rx):
  * ``nmse``     -- normalised MSE after the best complex scaling of x (:87-89),
  * ``gain_ana`` -- beamforming gain with 2-bit quantised beams (Quantize_PS, :95-99, :103),
  * ``gain_dig`` -- beamforming gain with the unquantised unit beams (:100-104),
  * ``proj_err`` -- rank-one projection error (:107-115).
The gauge of the singular vectors ``gain_ana`` quantises is the beamformer's (numpy's zgesdd; see
include/ace.h).  A realisation whose x or g is all zero or not finite returns nmse = 1,
proj_err = 1, both gains 0 and the status bit ACE_ST_EVAL_DEGENERATE (the reference gives NaN there).

Entry points (no CPU fallback -- every call runs ``evaluate_kernel`` on the GPU):
  * ``evaluate_host(X, G, tx, rx)`` -- numpy arrays.
  * ``evaluate_batch(X, G, tx, rx)`` -- device tensors already in HBM; no host copy.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import LIB, check, ACE_ST_EVAL_DEGENERATE

METRICS = ("nmse", "gain_ana", "gain_dig", "proj_err")   # column order of the C-ABI's metrics [batch][4]


@dataclass
class EvalResult:
    nmse: object       # [batch] float64
    gain_ana: object   # [batch] float64
    gain_dig: object   # [batch] float64
    proj_err: object   # [batch] float64
    status: object     # [batch] uint32 (host) / int32 (device): ACE_ST_EVAL_DEGENERATE, ACE_ST_BF_NOCONV
    metrics: object = None   # [batch][4], the four columns above as one array (views)

    @property
    def degenerate(self):
        return (self.status & ACE_ST_EVAL_DEGENERATE) != 0


def _result(metrics, status) -> EvalResult:
    return EvalResult(metrics[:, 0], metrics[:, 1], metrics[:, 2], metrics[:, 3], status, metrics)


def _shape(shape, tx, rx):
    if len(shape) != 2 or shape[1] != tx * rx:
        raise ValueError(f"X and G must be [batch][tx*rx] = [batch][{tx * rx}], got {tuple(shape)}")
    return shape[0]


def evaluate_host(X, G, tx, rx) -> EvalResult:
    """Evaluation_H for a batch on host arrays: X (estimates), G (truth) [batch][tx*rx] complex."""
    X = np.ascontiguousarray(np.atleast_2d(np.asarray(X, dtype=np.complex128)))
    G = np.ascontiguousarray(np.atleast_2d(np.asarray(G, dtype=np.complex128)))
    batch = _shape(X.shape, tx, rx)
    if G.shape != X.shape:
        raise ValueError(f"shape mismatch: X{X.shape} G{G.shape}")
    met = np.empty((batch, 4), np.float64)
    st = np.empty(batch, np.uint32)
    dp = lambda a: a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    check(LIB.ace_evaluate_host(batch, int(tx), int(rx), dp(X), dp(G), dp(met),
                                st.ctypes.data_as(C.POINTER(C.c_uint32))))
    return _result(met, st)


def evaluate_batch(X, G, tx, rx, *, out=None, stream=None) -> EvalResult:
    """Evaluation_H on device tensors: X, G [batch][tx*rx] complex128.  ``out``: an EvalResult of an earlier
    call with the same batch (its ``metrics`` [batch][4] float64 and ``status`` [batch] int32 tensors are
    reused).  Asynchronous on ``stream`` (default: the current stream); nothing is copied to the host."""
    import torch
    if not (X.is_cuda and G.is_cuda):
        raise ValueError("evaluate_batch needs device tensors")
    if X.dtype != torch.complex128 or G.dtype != torch.complex128:
        raise TypeError("X and G must be complex128")
    batch = _shape(tuple(X.shape), tx, rx)
    if tuple(G.shape) != tuple(X.shape):
        raise ValueError(f"shape mismatch: X{tuple(X.shape)} G{tuple(G.shape)}")
    X, G = X.contiguous(), G.contiguous()
    dev = X.device
    if out is None:
        met = torch.empty((batch, 4), dtype=torch.float64, device=dev)
        st = torch.empty(batch, dtype=torch.int32, device=dev)
    else:
        met, st = out.metrics, out.status
        if (tuple(met.shape) != (batch, 4) or met.dtype != torch.float64 or not met.is_contiguous()
                or tuple(st.shape) != (batch,) or st.dtype != torch.int32 or met.device != dev or st.device != dev):
            raise ValueError("out must hold metrics [batch][4] float64 and status [batch] int32 on X's device")
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    check(LIB.ace_evaluate_batch(batch, int(tx), int(rx), X.data_ptr(), G.data_ptr(), met.data_ptr(),
                                 st.data_ptr(), stream.cuda_stream))
    return _result(met, st)
