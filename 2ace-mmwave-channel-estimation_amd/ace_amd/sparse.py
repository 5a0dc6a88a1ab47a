"""Sparse recoveries on the angular dictionary: the baselines the reference's ``Vs_M.m`` draws next to the low-rank
ADMM recoveries.

  * ``dictionary_2d``      -- AD of Sparse_Channel_Formulation.m:136-143 on the cut grids of ``angular.dictionary``.
  * ``two_stage_setup``    -- the SVD compression rule of My_TwoStage_Recovery.m:78-100 (host, once per sweep point).
  * ``plomp_batch``        -- ``Method.PLOMP``: PhaseLift on P (``phaselift_batch``, unchanged), then OMP on C
                              (``omp.omp_batch``).  Recover_Channel.m:23-29 feeds it ``beams * AD`` and maps the result
                              back with ``AD * plomp_signal``: ``OmpResult.channel(AD)``.
  * ``plgamp_batch``       -- ``Method.PLGAMP``: the same PhaseLift stage, then EM-BG-GAMP on C
                              (``gamp.embgamp_batch``; My_TwoStage_Recovery.m:163-181), with the reference's OMP
                              fallback where EMBGAMP would raise.  ``two_stage_batch`` returns both methods from one
                              PhaseLift run, as the reference computes them.
  * ``perfect_phase_cs``   -- ``Method.PerfectPhaseCS`` (My_Conventional_CS.m) on coherent (complex) measurements:
                              ``solver="omp"`` is its ``OMP(A, y, s)`` branch (:81), ``solver="embgamp"`` its first
                              branch, EMBGAMP with learn_lambda (:71-79).
  * ``noisy_phase_cs``     -- ``Method.NoisyPhaseCS``: the same function on ``measurements_with_noisy_phase``
                              (``scenario.ScenarioResult.y_noisy``).

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


def dictionary_2d(tx, rx, NQ_t=None, NQ_r=None, search_deg=angular.SEARCH_DEG, ant_d=None):
    """AD [tx*rx][Qt*Qr]: column u Qr + v = kron(conj(A_tx[:, u]), A_rx[:, v]), u outer and v inner, over the cut
    grids of ``angular.dictionary`` (Sparse_Channel_Formulation.m:136-143).  Row t rx + r matches the synth's vec(H)
    order (element r + rx t), so a path on the grid is one column times gain sqrt(tx rx).  Returns
    (AD, sin grid of the tx side [Qt], sin grid of the rx side [Qr]).  ``ant_d``: the element spacing in metres
    (default the synth's)."""
    At, st, _ = angular.dictionary(tx, NQ_t, search_deg, ant_d)   # [Qt][tx], rows a(s)
    Ar, sr, _ = angular.dictionary(rx, NQ_r, search_deg, ant_d)
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


def _gamp_stage2(ts, sig, s, noise_power, n):
    """Stage 2 of PLGAMP on a stage-1 result: EMBGAMP(intSoln, C, optEM) with SNRdB = 10 log10(1 / noise_power),
    lambda = s / n, learn_lambda off; realisations the reference's try would leave through its catch
    (ACE_ST_GAMP_FAILED) receive OMP(C, intSoln, 1e-12), scattered into xhat.  (Looking for such realisations reads
    one flag back from the device.)"""
    import torch
    from .gamp import embgamp_batch
    res = embgamp_batch(ts.C, sig, 10.0 * math.log10(1.0 / float(noise_power)), s / n)
    failed = res.failed
    if bool(failed.any()):
        fb = omp_batch(ts.C, sig, ts.mCS, 1e-12, want_x=True)
        res.xhat = torch.where(failed[:, None], fb.x, res.xhat)
    return res


def plgamp_batch(Phi, meas_sq, s, noise_power, *, setup=None, **pl_kw):
    """``Method.PLGAMP`` (My_TwoStage_Recovery.m:163-181) for a batch: stage 1 as ``plomp_batch`` (``plomp_stage1``),
    stage 2 ``embgamp_batch(C, intSoln, 10 log10(1 / noise_power), s / n)``.  Returns the ``GampResult`` (xhat over
    the n columns of Phi; its ``channel(AD)`` is ``AD * plgamp_signal``); a realisation flagged ACE_ST_GAMP_FAILED
    carries the reference's fallback, ``omp_batch(C, intSoln, mCS, 1e-12)``, and keeps the flag."""
    ts, sig = plomp_stage1(Phi, meas_sq, s, setup=setup, **pl_kw)
    return _gamp_stage2(ts, sig, s, noise_power, Phi.shape[1])


def two_stage_batch(Phi, meas_sq, s, noise_power, *, tol=1e-12, max_atoms=None, setup=None, **pl_kw):
    """Both second stages on one PhaseLift run, as My_TwoStage_Recovery.m computes them: (``plomp_batch``'s
    OmpResult, ``plgamp_batch``'s GampResult)."""
    ts, sig = plomp_stage1(Phi, meas_sq, s, setup=setup, **pl_kw)
    kmax = ts.mCS if max_atoms is None else min(int(max_atoms), ts.mCS)
    return omp_batch(ts.C, sig, kmax, tol), _gamp_stage2(ts, sig, s, noise_power, Phi.shape[1])


def noisy_phase_cs(Phi, y_noisy, s, *, solver="omp", noise_power=None):
    """``Method.NoisyPhaseCS`` (Recover_Channel.m): ``My_Conventional_CS`` on ``measurements_with_noisy_phase``, the
    coherent measurements with every entry multiplied by its own CN(0,1) draw (Generate_Measurement.m:102-103;
    ``ScenarioResult.y_noisy``).  The recovery is ``perfect_phase_cs`` on that input, solver and limits included."""
    return perfect_phase_cs(Phi, y_noisy, s, solver=solver, noise_power=noise_power)


def perfect_phase_cs(Phi, y_complex, s, *, solver="omp", noise_power=None):
    """``Method.PerfectPhaseCS``: sparse recovery from coherent measurements y = Phi x + w (My_Conventional_CS.m).
    ``solver="omp"`` (the default) is the function's ``OMP(A, y, s)`` branch (:81), the fallback of its try: kmax = s,
    tol = 0; it returns an ``OmpResult``.  ``solver="embgamp"`` is its first branch (:71-79): EMBGAMP from the GAMP
    package the reference vendors, with SNRdB = 10 log10(1 / noise_power), lambda = s / n and learn_lambda on; it
    returns a ``GampResult``, and realisations flagged ACE_ST_GAMP_FAILED carry the OMP branch's solution, as the
    reference's catch gives.  Both kernels take atoms of length up to 256, so m = Phi.shape[0] <= 256."""
    m, n = Phi.shape
    if m > D_MAX:
        raise ValueError(f"perfect_phase_cs: Phi {m} x {n} has m > {D_MAX}, the sparse kernels' largest atom length")
    if solver == "omp":
        return omp_batch(Phi, y_complex, int(s), 0.0)
    if solver != "embgamp":
        raise ValueError(f"solver must be 'omp' or 'embgamp', got {solver!r}")
    if noise_power is None:
        raise ValueError("solver='embgamp' needs noise_power (optEM.SNRdB = 10 log10(1 / noise_power))")
    import torch
    from .gamp import embgamp_batch
    res = embgamp_batch(Phi, y_complex, 10.0 * math.log10(1.0 / float(noise_power)), s / n, learn_lambda=True)
    failed = res.failed
    if bool(failed.any()):
        fb = omp_batch(Phi, y_complex, int(s), 0.0, want_x=True)
        res.xhat = torch.where(failed[:, None], fb.x, res.xhat)
    return res
