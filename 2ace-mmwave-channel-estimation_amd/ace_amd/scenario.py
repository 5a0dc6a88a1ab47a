"""The reference's Monte-Carlo scenarios on the GPU (``ace_synth_scenario``, csrc/ace_scenario.hip):
``Generate_Channel.m`` and ``Generate_Measurement.m`` restated in full for a batch of realisations -- L paths or one
path with Rician NLOS paths, a searching area, on-grid angles, the iid or the combiner-coloured noise -- with every
measurement kind at its own scale: the coherent ``y``, the noisy-phase ``y_noisy``, the magnitudes ``B_raw`` and their
norm, and the normalised ``B``, ``X0``, ``Hn`` that ``ace_synth_channels`` returns.  The default configuration is
``ace_synth_channels``' scenario and draws its numbers; ``ace_amd.synth.scenario`` is the host mirror.

Entry point (no CPU fallback -- the call runs the kernels on the GPU):
  * ``scenario_batch(seed, first, count, tx, rx, A, cfg=None, W=None, want=(...))`` -- device tensors in and out.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

from ._lib import LIB, check, ScenarioCfg, scenario_cfg

ANT_MAX, M_MAX = 32, 4096   # the C-ABI's limits (include/ace.h)
OUTPUTS = ("vecH", "y", "y_noisy", "B_raw", "scale", "B", "X0", "Hn", "paths")


@dataclass
class ScenarioResult:
    """Device tensors of one call; an output that was not asked for is None."""
    vecH: object = None      # [count][n] complex128, the reference's scale, entry r + rx t = H[r][t]
    y: object = None         # [count][m] complex128: A vecH + noise
    y_noisy: object = None   # [count][m] complex128: y .* CN(0,1)
    B_raw: object = None     # [count][m] float64: |y|
    scale: object = None     # [count] float64: ||B_raw||
    B: object = None         # [count][m] float64: B_raw / scale
    X0: object = None        # [count][n] complex128: the perturbed start / scale
    Hn: object = None        # [count][n] complex128: vecH / scale
    paths: object = None     # [count][4 (L + Rk)] float64 (include/ace.h states the layout)
    noise_power: float = 0.0   # sigma2 = 10^(-snr_db/10), or the reference's 1e-10 with add_noise = 0


def rician_in_effect(cfg) -> int:
    """NLOS paths the channel has: ``rician_k`` when L == 1, else 0 (Generate_Channel.m:102-106)."""
    return int(cfg.rician_k) if int(cfg.L) == 1 else 0


def noise_power(cfg) -> float:
    return 10.0 ** (-float(cfg.snr_db) / 10.0) if cfg.add_noise else 1e-10


def scenario_batch(seed, first, count, tx, rx, A, cfg=None, W=None,
                   want=("vecH", "y", "y_noisy", "B_raw", "scale", "B", "X0", "Hn", "paths"), workspace=None,
                   stream=None, *, a_shared=None) -> ScenarioResult:
    """Realisations first .. first + count - 1 of the scenario ``cfg`` (a ``ScenarioCfg``; default:
    ``scenario_cfg()``) measured through A: a device complex128 tensor [m][n] or [1][m][n] (shared) or [count][m][n]
    (one codebook per realisation), n = tx rx.  ``W``: the combiners [Mr][rx] of noise model 1 (``beam_scan``'s rows,
    applied conjugated; m = Mt Mr).  ``want``: the outputs to form.  Asynchronous on ``stream`` (default: torch's
    current stream); nothing is read back.  ``a_shared=False`` with count == 1 takes the per-realisation product for
    a single [1][m][n] codebook (default: one leading codebook means shared).  ``workspace``: a ``solver.Workspace``
    (default: the package's shared one)."""
    import torch
    from .solver import _DEFAULT_WS
    cfg = scenario_cfg() if cfg is None else cfg
    if not isinstance(cfg, ScenarioCfg):
        raise TypeError("cfg must be a ScenarioCfg (scenario_cfg(...))")
    unknown = [k for k in want if k not in OUTPUTS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}; choose from {OUTPUTS}")
    if not A.is_cuda or A.dtype != torch.complex128:
        raise TypeError("A must be a complex128 device tensor")
    if not 1 <= tx <= ANT_MAX or not 1 <= rx <= ANT_MAX or count < 1 or first < 0:
        raise ValueError(f"tx and rx must be 1..{ANT_MAX}, count >= 1 and first >= 0 (got {tx}, {rx}, {count}, {first})")
    n = int(tx) * int(rx)
    if A.dim() == 2:
        A = A[None]
    if A.dim() != 3 or A.shape[2] != n or A.shape[0] not in (1, count):
        raise ValueError(f"A must be [m][{n}], [1][m][{n}] or [{count}][m][{n}], got {tuple(A.shape)}")
    if a_shared is None:
        a_shared = A.shape[0] == 1
    elif a_shared and A.shape[0] != 1:
        raise ValueError("a shared codebook is [m][n] or [1][m][n]")
    elif not a_shared and A.shape[0] != count:
        raise ValueError(f"codebooks per realisation are [{count}][m][n], got {tuple(A.shape)}")
    m = int(A.shape[1])
    if not 1 <= m <= M_MAX:
        raise ValueError(f"A must have 1..{M_MAX} rows, got {m}")
    dev = A.device
    A = A.contiguous()
    Mr = 0
    if W is not None:
        if not W.is_cuda or W.dtype != torch.complex128 or W.dim() != 2 or W.shape[1] != rx or W.device != dev:
            raise ValueError(f"W must be a complex128 [Mr][{rx}] tensor on A's device")
        W = W.contiguous()
        Mr = int(W.shape[0])
    elif cfg.noise_model == 1:
        raise ValueError("noise model 1 needs the combiners W")
    P = int(cfg.L) + rician_in_effect(cfg)
    shapes = {"vecH": ((count, n), torch.complex128), "y": ((count, m), torch.complex128),
              "y_noisy": ((count, m), torch.complex128), "B_raw": ((count, m), torch.float64),
              "scale": ((count,), torch.float64), "B": ((count, m), torch.float64),
              "X0": ((count, n), torch.complex128), "Hn": ((count, n), torch.complex128),
              "paths": ((count, 4 * P), torch.float64)}
    out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in OUTPUTS if k in want}
    nbytes = int(LIB.ace_synth_scenario_workspace_size(C.byref(cfg), count, m, tx, rx, Mr)) + 256
    ws = (workspace or _DEFAULT_WS).get(nbytes, dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    ptr = lambda k: out[k].data_ptr() if k in out else None   # noqa: E731
    check(LIB.ace_synth_scenario(C.byref(cfg), seed, first, count, m, tx, rx, A.data_ptr(), int(a_shared),
                                 None if W is None else W.data_ptr(), Mr, *[ptr(k) for k in OUTPUTS],
                                 ws.data_ptr(), ws.numel(), stream.cuda_stream))
    return ScenarioResult(noise_power=noise_power(cfg), **out)
