"""Sparse recoveries on the angular dictionary: the baselines the reference's ``Vs_M.m`` draws next to the low-rank
ADMM recoveries.

  * ``dictionary_2d``      -- AD of Sparse_Channel_Formulation.m:136-143 on the cut grids of ``angular.dictionary``.
  * ``two_stage_setup``    -- the SVD compression rule of My_TwoStage_Recovery.m:78-100 (host, once per sweep point).
  * ``plomp_batch``        -- ``Method.PLOMP``: PhaseLift on P (``phaselift_batch``, unchanged), then OMP on C
                              (``omp.omp_batch``).  Recover_Channel.m:23-29 feeds it ``beams * AD`` and maps the result
                              back with ``AD * plomp_signal``: ``OmpResult.channel(AD)``.
  * ``perfect_phase_cs``   -- ``Method.PerfectPhaseCS``: the ``OMP(A, y, s)`` branch of My_Conventional_CS.m:81 on
                              coherent (complex) measurements.

``OMP.m`` is not in the reference tree (it belongs to the external CoSaMP_OMP toolbox); ``omp.py`` says what is
implemented in its place.  With the reference's tolerance 1e-12 on noisy data OMP does not stop on the residual: it
runs until it has picked ``mCS`` atoms (the intermediate vector has mCS entries, so mCS independent atoms reproduce it
to rounding, whatever they are).  That is what the "faithful" setting ``max_atoms=None`` does; ``max_atoms = 2 s`` is
the setting a user of a sparse solver would choose.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import angular
from .omp import D_MAX, OmpResult, omp_batch


def dictionary_2d(tx, rx, NQ_t=None, NQ_r=None, search_deg=angular.SEARCH_DEG):
    """AD [tx*rx][Qt*Qr]: column u Qr + v = kron(conj(A_tx[:, u]), A_rx[:, v]), u outer and v inner, over the cut
    grids of ``angular.dictionary`` (Sparse_Channel_Formulation.m:136-143).  Row t rx + r matches the synth's vec(H)
    order (element r + rx t), so a path on the grid is one column times gain sqrt(tx rx).  Returns
    (AD, sin grid of the tx side [Qt], sin grid of the rx side [Qr])."""
    At, st, _ = angular.dictionary(tx, NQ_t, search_deg)   # [Qt][tx], rows a(s)
    Ar, sr, _ = angular.dictionary(rx, NQ_r, search_deg)
    AD = np.conj(At)[:, None, :, None] * Ar[None, :, None, :]          # [u][v][t][r]
    return np.ascontiguousarray(AD.reshape(len(st) * len(sr), tx * rx).T), st, sr


def _round(x):
    """MATLAB's round for the positive arguments of the rule (halves away from zero)."""
    return int(math.floor(x + 0.5))


@dataclass
class TwoStage:
    P: object    # [m][mCS] complex128: U sqrt(S), the phase-retrieval matrix of stage 1
    C: object    # [mCS][n] complex128: sqrt(S) V^H, the dictionary of stage 2
    mCS: int

    def to(self, device):
        import torch
        up = lambda a: a if not isinstance(a, np.ndarray) else torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        return TwoStage(up(self.P), up(self.C), self.mCS)


def two_stage_setup(Phi, s) -> TwoStage:
    """The compression of My_TwoStage_Recovery.m:78-100 for Phi [m][n] (numpy) and sparsity s, as it stands there:
    thin SVD; mCS_required = round(1.75 s log(n / s)); mCS starts at min(mCS_required, number of singular values)
    - 1, grows until the first mCS singular values hold 80 % of the singular-value SUM, then grows while
    round(1.75 mCS log(mCS)) < m; P = U sqrt(S), C = sqrt(S) V^H on the first mCS triplets.  Raises when mCS
    exceeds the OMP kernel's atom length."""
    Phi = np.asarray(Phi, dtype=np.complex128)
    m, n = Phi.shape
    U, dS, Vh = np.linalg.svd(Phi, full_matrices=False)
    nS = len(dS)
    mCS = min(_round(1.75 * s * math.log(n / s)), nS) - 1
    tot = dS.sum()
    while dS[:mCS].sum() / tot < 0.80 and mCS < nS:
        mCS += 1
    while mCS < nS and _round(1.75 * mCS * math.log(mCS)) < m:   # (mCS >= 1 here: the 80 % loop left 0 behind)
        mCS += 1
    if mCS > D_MAX:
        raise ValueError(f"two_stage_setup: Phi {m} x {n} with s = {s} compresses to mCS = {mCS} > {D_MAX}, "
                         f"the OMP kernel's largest atom length")
    rt = np.sqrt(dS[:mCS])
    return TwoStage(U[:, :mCS] * rt[None, :], rt[:, None] * Vh[:mCS], int(mCS))


def _setup_for(Phi, s, setup):
    if setup is None:
        setup = two_stage_setup(Phi.cpu().numpy(), s)
    return setup.to(Phi.device)


def plomp_stage1(Phi, meas_sq, s, *, setup=None, **pl_kw):
    """Stage 1 of the two-stage recovery: (TwoStage on the device, intSoln [batch][mCS]).  ``setup``: a
    ``two_stage_setup`` result to reuse (the SVD runs once per sweep point, on the host).  ``pl_kw`` go to
    ``phaselift_batch`` (maxIts, tol, restart, lam: the reference's 4000, 1e-10, 200, 0.05 by default); its ``sig`` is
    sqrt(eVal) times the leading eigenvector (:147-152).  A shape PhaseLift refuses raises PhaseLift's own error."""
    from .phaselift import phaselift_batch
    ts = _setup_for(Phi, s, setup)
    return ts, phaselift_batch(ts.P, meas_sq, **pl_kw).sig


def plomp_batch(Phi, meas_sq, s, *, tol=1e-12, max_atoms=None, setup=None, **pl_kw) -> OmpResult:
    """``Method.PLOMP`` (My_TwoStage_Recovery.m) for a batch: Phi [m][n] complex128 (``beams * AD``), meas_sq
    [batch][m] float64 (the squared magnitudes), device tensors.  Stage 1: PhaseLift on P.  Stage 2:
    ``omp_batch(C, intSoln, kmax = max_atoms or mCS, tol)``.  Returns the sparse result (indices into the n columns
    of Phi); its ``channel(AD)`` is ``AD * plomp_signal``.  The columns of C are not unit-norm and, like the
    reference's call, the selection does not normalise them."""
    ts, sig = plomp_stage1(Phi, meas_sq, s, setup=setup, **pl_kw)
    kmax = ts.mCS if max_atoms is None else min(int(max_atoms), ts.mCS)
    return omp_batch(ts.C, sig, kmax, tol)


def perfect_phase_cs(Phi, y_complex, s) -> OmpResult:
    """``Method.PerfectPhaseCS``: sparse recovery from coherent measurements y = Phi x + w.  This is the
    ``OMP(A, y, s)`` branch of My_Conventional_CS.m:81, i.e. the reference's fallback: the EM-GAMP solver it tries
    first (EMBGAMP, an external package) is not built here.  kmax = s, tol = 0.  The kernel takes atoms of length
    up to 256, so it needs m = Phi.shape[0] <= 256."""
    m, n = Phi.shape
    if m > D_MAX:
        raise ValueError(f"perfect_phase_cs: Phi {m} x {n} has m > {D_MAX}, the OMP kernel's largest atom length")
    return omp_batch(Phi, y_complex, int(s), 0.0)
