"""Monte-Carlo sweep over the number of measurements: the reference's ``Vs_M`` loop
(Numerical_Simulation/Vs_M.m:163-226: synthesise, recover, ``Evaluation_H``, average) for the two
ADMM methods, with every step on the GPU.

Per sweep point M: a shared phase-code codebook and the channels from the device synth
(``solver.synth_problem``), the recovery pipeline on per-realisation train partitions
(``pipeline.infer_low_rank_pipeline_batch``) and ``evaluate.evaluate_batch`` against the synthesised
vec(H).  Only the [count][4] metrics and the status words leave the device.

Shards.  The pipeline's results depend, at rounding level, on the batch a realisation is solved in: its
r-column stages take the int8 digit-plane applies from 256 vectors (batch x r) on and f64 GEMMs below, and
the rank-one retry solves the failing realisations as a sub-batch of their own.  The sweep
therefore always solves whole chunks of ``chunk`` consecutive realisations on the grid of the sweep's own
realisation index (realisation i belongs to chunk i // chunk, whatever ``first`` and ``count``), and keeps
the rows asked for: a realisation's metrics are a function of (seed, M, i, chunk) alone, and any shard
reproduces its rows of the full run bit for bit.

``vs_snr`` is the sweep over SNR of ``Vs_SNR.m`` in the reference's own scenario (``scenario.scenario_batch``), on the
same chunk grid.  ``vs_sr`` is ``VS_SR_par.m``: the mean angle estimation error against the number of measurements per
searching area.  The sparse recoveries can be scored with the reference's own ``Evaluation_Recovery``
(``recovery_eval.evaluate_recovery_batch``, 15 columns): ``vs_sr`` always does, ``vs_m_sparse`` and ``vs_snr`` with
``columns="recovery"``.
"""
from __future__ import annotations

import math

import numpy as np

from ._lib import pipeline_cfg, ACE_ST_EVAL_DEGENERATE
from .evaluate import METRICS, evaluate_batch

METHODS = ("A2only", "A2nuclear")
CHUNK = 64   # realisations per pipeline call (the default of vs_m's ``chunk``)


def vs_m(tx, rx, M_list, count, *, method="A2only", snr_db=30.0, L=3, seed, first=0, maxiter=None,
         device=None, chunk=CHUNK) -> dict:
    """Evaluation_H metrics of ``count`` recoveries at each M of ``M_list``.

    Realisation b of the call is realisation ``first + b`` of the sweep: its channel, its noise and its
    train partitions (the build's counter RNG, seed ``seed``, stream ``(first + b) * restarts + restart``:
    what the pipeline draws for ``train_idx = NULL`` on a batch that starts at realisation 0) depend on that
    index alone, and the codebook of a sweep point on ``seed`` and M, so shards of a sweep compose (see the
    module text for ``chunk``; a call whose range is not chunk-aligned solves up to ``chunk - 1`` extra
    realisations at each end and drops them on the device).  ``maxiter`` caps every ADMM stage (default: the
    reference's 500).

    Returns a dict: ``M`` [nM], ``metrics`` [nM][count][4] (columns ``evaluate.METRICS``), ``status``
    [nM][count] (the evaluator's), ``mean`` [nM][4] (the reference's
    mean(Evaluation) over the realisations, degenerate ones included with nmse = proj_err = 1 and zero
    gains) and ``n_degenerate`` [nM].  A sweep point the pipeline refuses (e.g. floor(0.95 M) < min(20, M)
    train rows) raises the pipeline's own error (AceError, or the ValueError of
    ``infer_low_rank_pipeline_batch`` for a configuration its workspace query rejects); it is not masked."""
    import torch
    from .engine import randperm
    from .pipeline import infer_low_rank_pipeline_batch
    from .solver import VARIANTS, synth_problem
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if tx != rx:
        # the synth vectorises its Nr x Nt channel with rx leading (k = r + rx t, Generate_Channel.m), the
        # pipeline and the evaluator read n-vectors with tx leading (k = i + tx j): the two agree for square arrays
        raise ValueError(f"vs_m needs tx == rx (got {tx} x {rx}): the synth's vec(H) order has rx leading")
    count, first, chunk = int(count), int(first), int(chunk)
    if count < 1 or first < 0 or chunk < 1:
        raise ValueError("count and chunk must be >= 1 and first >= 0")
    Ms = [int(M) for M in M_list]
    dev = torch.device("cuda" if device is None else device)
    cfg = pipeline_cfg(VARIANTS[method])
    R = cfg.restarts
    kw = {} if maxiter is None else {"maxiter": int(maxiter)}
    metrics = np.empty((len(Ms), count, 4), np.float64)
    status = np.empty((len(Ms), count), np.uint32)
    end = first + count
    for k, M in enumerate(Ms):
        mt = math.floor(M * cfg.cc_frac)
        for c0 in range(first // chunk * chunk, end, chunk):
            A, B, _, H = synth_problem(seed, c0, chunk, M, tx, rx, L=L, snr_db=snr_db, device=dev)
            tr = np.stack([np.stack([randperm(seed, (c0 + b) * R + i, M, mt) for i in range(R)])
                           for b in range(chunk)])
            rec = infer_low_rank_pipeline_batch(A, B, tx, rx, tr, variant=method, restarts=R, **kw)
            ev = evaluate_batch(rec.X, H, tx, rx)
            lo, hi = max(first, c0), min(end, c0 + chunk)   # the rows of this chunk the call asked for
            rows = slice(lo - first, hi - first)
            metrics[k, rows] = ev.metrics[lo - c0:hi - c0].cpu().numpy()
            status[k, rows] = ev.status[lo - c0:hi - c0].cpu().numpy().view(np.uint32)
    return {"M": np.asarray(Ms, np.int64), "metrics": metrics, "status": status,
            "mean": metrics.mean(axis=1), "n_degenerate": ((status & ACE_ST_EVAL_DEGENERATE) != 0).sum(axis=1),
            "columns": METRICS}


def vs_m_minl2(tx, rx, M_list, count, *, snr_db=30.0, L=3, seed, first=0, maxiter=None, device=None,
               chunk=CHUNK) -> dict:
    """``vs_m`` for the recovery without a prior (``minl2.infer_min_l2_batch``: ``Method.ADMM`` of Vs_M.m): the same
    chunk grid, codebook, channels and noise draws, so the curve stands next to ``vs_m``'s.  One train partition per
    chunk, ``engine.randperm(seed, c0, M, ceil(0.95 M))`` with c0 the chunk's first realisation: a realisation's
    metrics are a function of (seed, M, i, chunk) alone and shards compose as ``vs_m``'s do.

    Returns ``vs_m``'s keys (the status words are the evaluator's or-ed with the recovery's) plus ``r_used`` and
    ``quality`` [nM][count] and ``stage_iters`` [nM][count][3]."""
    import torch
    from .engine import randperm
    from .minl2 import infer_min_l2_batch, train_count
    from .solver import synth_problem
    if tx != rx:
        raise ValueError(f"vs_m_minl2 needs tx == rx (got {tx} x {rx}): the synth's vec(H) order has rx leading")
    count, first, chunk = int(count), int(first), int(chunk)
    if count < 1 or first < 0 or chunk < 1:
        raise ValueError("count and chunk must be >= 1 and first >= 0")
    Ms = [int(M) for M in M_list]
    dev = torch.device("cuda" if device is None else device)
    kw = {} if maxiter is None else {"maxiter": int(maxiter)}
    metrics = np.empty((len(Ms), count, 4), np.float64)
    status = np.empty((len(Ms), count), np.uint32)
    r_used = np.empty((len(Ms), count), np.int32)
    quality = np.empty((len(Ms), count), np.float64)
    stage_iters = np.empty((len(Ms), count, 3), np.int32)
    end = first + count
    for k, M in enumerate(Ms):
        mt = train_count(M)
        for c0 in range(first // chunk * chunk, end, chunk):
            A, B, _, H = synth_problem(seed, c0, chunk, M, tx, rx, L=L, snr_db=snr_db, device=dev)
            rec = infer_min_l2_batch(A, B, randperm(seed, c0, M, mt), **kw)
            ev = evaluate_batch(rec.X, H, tx, rx)
            lo, hi = max(first, c0), min(end, c0 + chunk)   # the rows of this chunk the call asked for
            rows, sel = slice(lo - first, hi - first), slice(lo - c0, hi - c0)
            metrics[k, rows] = ev.metrics[sel].cpu().numpy()
            status[k, rows] = (ev.status[sel] | rec.status[sel]).cpu().numpy().view(np.uint32)
            r_used[k, rows] = rec.r_used[sel].cpu().numpy()
            quality[k, rows] = rec.quality[sel].cpu().numpy()
            stage_iters[k, rows] = rec.stage_iters[sel].cpu().numpy()
    return {"M": np.asarray(Ms, np.int64), "metrics": metrics, "status": status,
            "mean": metrics.mean(axis=1), "n_degenerate": ((status & ACE_ST_EVAL_DEGENERATE) != 0).sum(axis=1),
            "columns": METRICS, "r_used": r_used, "quality": quality, "stage_iters": stage_iters}


SWEEP1_SEED = 0x9E3779B9   # added to the seed for sweep pattern 1's noise: patterns 1 and 2 draw independently


def _dense_z(r):
    """The sparse vector of a recovery [batch][N] on the device: a GAMP result's ``xhat``, an OMP result's support and
    coefficients scattered into zeros (coef is 0 past count)."""
    import torch
    if hasattr(r, "xhat"):
        return r.xhat.contiguous()
    if r.x is not None:
        return r.x.contiguous()
    z = torch.zeros((r.idx.shape[0], r.N, 2), dtype=torch.float64, device=r.idx.device)
    z.scatter_add_(1, r.idx.clamp(min=0).long()[:, :, None].expand(-1, -1, 2), torch.view_as_real(r.coef))
    return torch.view_as_complex(z)


def _sweep_picks(Hraw, tx, rx, Mt, Mr, snr_db, seed, first, search_deg):
    """[batch][2][2] int32 on the device: (ind_F, ind_W) zero-based of the reference's sweep pattern 1 and pattern 2
    (Evaluation_Recovery.m:232-233).  The two run the same quantised beams (``angular.directional_beams``) on
    independent noise draws: pattern 2 ``angular.beam_sweep``'s at ``seed``, pattern 1 at ``seed + SWEEP1_SEED``."""
    import torch
    from . import angular
    pk = []
    for sd in (seed + SWEEP1_SEED, seed):
        _, _, p, q = angular.beam_sweep(Hraw, tx, rx, Mt, Mr, snr_db=snr_db, seed=sd, first=first, search_deg=search_deg)
        pk.append(torch.stack([p, q], dim=1))
    return torch.stack(pk, dim=1).to(torch.int32).contiguous()


def _check_columns(columns):
    if columns not in ("h", "recovery"):
        raise ValueError(f"columns must be 'h' or 'recovery', got {columns!r}")
    return columns == "recovery"


SPARSE = ("plomp", "plomp_2s", "perfect_cs")
SPARSE_GAMP = ("plgamp", "perfect_cs_gamp")
SPARSE_PRGAMP = ("prgamp",)


def vs_m_sparse(tx, rx, M_list, count, *, s=None, snr_db=30.0, L=3, seed, first=0, pl_maxits=4000, tol=1e-12,
                device=None, chunk=CHUNK, gamp=False, prgamp=False, max_try=100, columns="h") -> dict:
    """The sparse recoveries of ``sparse.py`` on ``vs_m``'s sweep: the same chunk grid, codebook, channels and noise
    draws (``synth_problem`` at (seed, M, realisation index)), so the curves stand next to ``vs_m``'s.  Per M and
    realisation, the four ``evaluate_batch`` columns ([nM][count][4] each, keys ``SPARSE``) of

      * ``plomp``      -- ``sparse.plomp_batch`` on Phi = A AD and the squared measurements at the synth's own scale
                          (Recover_Channel.m:25; not the B / ||B|| InferADMM sees) with ``max_atoms = mCS``: the
                          reference's call, whose tolerance 1e-12 never stops OMP on noisy data;
      * ``plomp_2s``   -- the same PhaseLift solution with ``max_atoms = 2 s``;
      * ``perfect_cs`` -- ``sparse.perfect_phase_cs`` on the coherent measurements A h + w with the w whose modulus
                          the magnitude measurements are (``synth.measurements_complex``, built on the host and
                          uploaded), where M <= 256; NaN beyond (the OMP kernel's atom length).

    ``gamp=True`` adds the EM-BG-GAMP baselines on the same chunk grid and draws (keys ``SPARSE_GAMP``; the keys of
    ``SPARSE`` and their values do not change):

      * ``plgamp``          -- ``Method.PLGAMP``: the PhaseLift solution ``plomp`` uses, then ``gamp.embgamp_batch`` on C
                               with noise_power = 10^(-snr_db / 10) and the reference's OMP fallback;
      * ``perfect_cs_gamp`` -- ``sparse.perfect_phase_cs(..., solver="embgamp")`` on ``perfect_cs``'s measurements;

    with ``status_<key>`` (the evaluator's bits or-ed with the GAMP stage's) and ``em_iters_<key>`` [nM][count].

    ``prgamp=True`` adds the direct compressive phase retrieval ``Method.PRGAMP`` (key ``SPARSE_PRGAMP``; every other
    key and value is unchanged):

      * ``prgamp`` -- ``prgamp.prgamp_batch`` on Phi = A AD and the magnitude measurements at the synth's own scale
                      (MyCPR.m:110-120: sparse_rat = s / n with n the dictionary size, SNRdBinit 20, SNRdB 25, nitEM
                      50), scored like ``plomp``, where M <= 256; NaN beyond (the kernel's row limit).  The restart
                      draws come from the counter generator at (seed, realisation index), so shards compose.

    with ``status_prgamp`` (the evaluator's bits or-ed with the solver's) and ``tries_prgamp`` [nM][count] (numTry).
    ``max_try``: the restarts per realisation, default the reference's 100.  The draws cost 16 chunk max_try Qt Qr bytes
    per sweep point: 105 MB at the default chunk of 64, a 32 x 32 dictionary and 100 tries (1.7 GB at a 16384-atom
    dictionary), and a realisation that never reaches the stop level runs all of them.

    ``s``: the sparsity handed to both (default L, what Vs_M.m passes).  Also returned: ``mCS`` [nM], the status
    words of the three evaluations or-ed with the OMP stage's (``status_<key>``), the OMP stage's counts (``count_<key>``),
    ``gain_percsi_ana`` [nM][count] (``evaluate_batch(H, H)``: the H scored is ``vs_m``'s) and the means.  Only
    metrics, counts and status words leave the device.

    ``columns="recovery"`` adds the reference's own score of these methods, ``Evaluation_Recovery``
    (``recovery_eval.evaluate_recovery_batch``): per method ``recovery_<key>`` [nM][count][15] (columns
    ``columns_recovery`` = ``recovery_eval.METRICS_RECOVERY``) and ``status_recovery_<key>``, against the channel at the
    synth's own scale (the scale of the measurements the recoveries see; MSE_H is not scale-free), the synth's true
    angles and, for the sweep columns, ``angular.beam_sweep`` with round(sqrt(M)) beams per side run twice on independent
    noise (patterns 1 and 2).  Every other key and value is bit-identical to the default ``columns="h"``.

    Cost.  The two-stage setup runs one host SVD of Phi (M x Qt Qr) per sweep point.  PhaseLift dominates: one
    TFOCS iteration per realisation is an eigendecomposition of an mCS x mCS matrix and two products with P, and
    the reference's ``pl_maxits`` = 4000 at mCS around 150 makes a sweep point of 64 realisations take minutes, a
    full 16 x 16 curve tens of minutes; lower ``pl_maxits`` to bound it and say so next to the numbers."""
    import torch
    from . import sparse, synth
    from . import prgamp as prgamp_mod
    from .solver import synth_problem
    if tx != rx:
        raise ValueError(f"vs_m_sparse needs tx == rx (got {tx} x {rx}): the synth's vec(H) order has rx leading")
    want_rec = _check_columns(columns)
    count, first, chunk = int(count), int(first), int(chunk)
    if count < 1 or first < 0 or chunk < 1:
        raise ValueError("count and chunk must be >= 1 and first >= 0")
    s = int(L if s is None else s)
    Ms = [int(M) for M in M_list]
    dev = torch.device("cuda" if device is None else device)
    n = tx * rx
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    AD = up(sparse.dictionary_2d(tx, rx)[0])
    out = {k: np.full((len(Ms), count, 4), np.nan) for k in SPARSE}
    stat = {k: np.zeros((len(Ms), count), np.uint32) for k in SPARSE}
    cnt = {k: np.zeros((len(Ms), count), np.int32) for k in SPARSE}
    keys_g = SPARSE_GAMP if gamp else ()
    out.update({k: np.full((len(Ms), count, 4), np.nan) for k in keys_g})
    stat.update({k: np.zeros((len(Ms), count), np.uint32) for k in keys_g})
    emi = {k: np.zeros((len(Ms), count), np.int32) for k in keys_g}
    keys_p = SPARSE_PRGAMP if prgamp else ()
    out.update({k: np.full((len(Ms), count, 4), np.nan) for k in keys_p})
    stat.update({k: np.zeros((len(Ms), count), np.uint32) for k in keys_p})
    tries = {k: np.zeros((len(Ms), count), np.int32) for k in keys_p}
    noise_power = 10.0 ** (-snr_db / 10.0)
    percsi = np.empty((len(Ms), count), np.float64)
    mcs = np.empty(len(Ms), np.int64)
    end = first + count
    rec, rec_st = {}, {}
    if want_rec:
        from . import angular, recovery_eval
        rec = {k: np.full((len(Ms), count, recovery_eval.NCOL), np.nan) for k in out}
        rec_st = {k: np.zeros((len(Ms), count), np.uint32) for k in out}
        tb = recovery_eval.recovery_tables(tx, rx)
    for k, M in enumerate(Ms):
        setup, Phi, Ah = None, None, synth.codebook(seed, M, n)
        if want_rec:
            nb_sw = max(1, int(round(math.sqrt(M))))
            sw = recovery_eval.sweep_tables(tx, rx, nb_sw, nb_sw)
        for c0 in range(first // chunk * chunk, end, chunk):
            A, B, _, H = synth_problem(seed, c0, chunk, M, tx, rx, L=L, snr_db=snr_db, device=dev)
            if setup is None:
                Phi = (A[0] @ AD).contiguous()
                setup = sparse.two_stage_setup(Phi.cpu().numpy(), s).to(dev)
                mcs[k] = setup.mCS
            # the synth hands out B / ||B|| (what InferADMM sees); Recover_Channel.m:25 passes the measurements as
            # they are, and PhaseLift's trace weight lambda = 0.05 is not scale-free: undo the normalisation with
            # ||B|| = ||H|| / ||H / ||B|| || from the host copy of the channel
            Hh = np.stack([synth.channel(seed, c0 + b, tx, rx, L) for b in range(chunk)])
            nb = up(np.linalg.norm(Hh, axis=1)) / torch.linalg.vector_norm(H, dim=1)
            Braw = B * nb[:, None]
            ts, sig = sparse.plomp_stage1(Phi, Braw * Braw, s, setup=setup, maxIts=int(pl_maxits))
            res = {"plomp": sparse.omp_batch(ts.C, sig, ts.mCS, tol),
                   "plomp_2s": sparse.omp_batch(ts.C, sig, min(2 * s, ts.mCS), tol)}
            if M <= sparse.D_MAX:
                y = np.stack([synth.measurements_complex(seed, c0 + b, Ah, Hh[b], snr_db) for b in range(chunk)])
                res["perfect_cs"] = sparse.perfect_phase_cs(Phi, up(y), s)
                if gamp:
                    res["perfect_cs_gamp"] = sparse.perfect_phase_cs(Phi, up(y), s, solver="embgamp",
                                                                     noise_power=noise_power)
            if gamp:
                res["plgamp"] = sparse._gamp_stage2(ts, sig, s, noise_power, Phi.shape[1])
            if prgamp and M <= prgamp_mod.M_MAX:
                res["prgamp"] = prgamp_mod.prgamp_batch(Phi, Braw.contiguous(), s / Phi.shape[1], seed=seed, first=c0,
                                                        max_try=int(max_try))
            lo, hi = max(first, c0), min(end, c0 + chunk)   # the rows of this chunk the call asked for
            rows, sel = slice(lo - first, hi - first), slice(lo - c0, hi - c0)
            percsi[k, rows] = evaluate_batch(H, H, tx, rx).gain_ana[sel].cpu().numpy()
            res_aux = {}
            for name, r in res.items():
                ev = evaluate_batch(r.channel(AD), H, tx, rx)
                out[name][k, rows] = ev.metrics[sel].cpu().numpy()
                # the evaluator's bits and the OMP stage's (ACE_ST_EVAL_DEGENERATE there: a non-finite PhaseLift output)
                stat[name][k, rows] = (ev.status[sel] | r.status[sel]).cpu().numpy().view(np.uint32)
                if want_rec:
                    if "Hraw" not in res_aux:
                        tru = [synth.paths(seed, c0 + b, L) for b in range(chunk)]
                        res_aux["Hraw"] = up(Hh)
                        res_aux["aod"], res_aux["aoa"] = up(np.stack([t[0] for t in tru])), up(np.stack([t[1] for t in tru]))
                        res_aux["picks"] = _sweep_picks(res_aux["Hraw"], tx, rx, nb_sw, nb_sw, snr_db, seed, c0,
                                                        angular.SEARCH_DEG)
                    rv = recovery_eval.evaluate_recovery_batch(_dense_z(r), res_aux["Hraw"], res_aux["aod"], res_aux["aoa"],
                                                               tb, noise_power=noise_power, picks=res_aux["picks"], sweep=sw)
                    rec[name][k, rows] = rv.metrics[sel].cpu().numpy()
                    rec_st[name][k, rows] = (rv.status[sel] | r.status[sel]).cpu().numpy().view(np.uint32)
                if name in tries:
                    tries[name][k, rows] = r.counts[sel, 0].cpu().numpy()
                elif name in emi:
                    emi[name][k, rows] = r.em_iters[sel].cpu().numpy()
                else:
                    cnt[name][k, rows] = r.count[sel].cpu().numpy()
    return {"M": np.asarray(Ms, np.int64), "mCS": mcs, "s": s, **out, "columns": METRICS, "gain_percsi_ana": percsi,
            **{f"status_{k}": v for k, v in stat.items()}, **{f"count_{k}": v for k, v in cnt.items()},
            **{f"em_iters_{k}": v for k, v in emi.items()}, **{f"tries_{k}": v for k, v in tries.items()}, "mean": {k: v.mean(axis=1) for k, v in out.items()},
            **_recovery_keys(rec, rec_st)}


def _recovery_keys(rec, rec_st):
    """The keys ``columns="recovery"`` adds to a sweep's dict (none for the default)."""
    if not rec:
        return {}
    from .recovery_eval import METRICS_RECOVERY
    return {**{f"recovery_{k}": v for k, v in rec.items()}, **{f"status_recovery_{k}": v for k, v in rec_st.items()},
            "columns_recovery": METRICS_RECOVERY, "mean_recovery": {k: v.mean(axis=1) for k, v in rec.items()}}


BASELINES = ("gain_percsi_ana", "gain_percsi_dig", "aoda_err_est", "gain_est_aoda", "gain_sweep", "aoda_err_sweep")


def vs_m_baselines(tx, rx, M_list, count, *, method="A2only", snr_db=30.0, L=3, seed, first=0, maxiter=None,
                   device=None, chunk=CHUNK) -> dict:
    """``vs_m`` with the yardsticks of Evaluation_Recovery.m beside it: the same loop on the same chunk grid (the
    four Evaluation_H columns equal ``vs_m``'s bit for bit, and shards compose the same way), plus, per M and
    realisation ([nM][count] each, keys ``BASELINES``):

      * ``gain_percsi_ana``, ``gain_percsi_dig`` -- ``evaluate_batch(H, H)``: the quantised and the unit-beam
        gain of the true channel's own singular pair (:195-203, :268-269);
      * ``aoda_err_est`` -- (|dAoD| + |dAoA|) / 2 of ``angular.estimate_angles`` on the recovered channel against
        the nearest true path, degrees (:135-146);
      * ``gain_est_aoda`` -- |w^H H f| on the true H with the 2-bit quantised steering vectors at the estimated
        angles (:226-229, :271);
      * ``gain_sweep``, ``aoda_err_sweep`` -- the same two numbers for the pair ``angular.beam_sweep`` picks
        with Mt = Mr = round(sqrt(M)) beams (about the same number of probes) at ``snr_db`` (:232-259, :273).

    The gains are in ``gain_ana``'s unit, so that the columns divide into each other: the true H as InferADMM
    sees it (divided by ||B||) and quantised beams with Quantize_PS's own 1 / sqrt(antennas) each, which is what
    ``evaluate_batch`` applies to ``gain_ana`` (the scan runs on the unit-modulus beams, exact powers of j, and
    the modulus is divided by sqrt(tx rx)).  The sweep itself, whose noise is
    absolute, runs on the channel at the synth's own scale (``synth.channel``).  The realisation's recovery runs
    once; each gain is read off one beam scan of the true H; only per-realisation metrics leave the device.  A
    realisation whose estimate is degenerate (a non-finite recovery) gets ``gain_est_aoda`` 0 and ``aoda_err_est``
    = the width of the angular range, so that means stay finite.  Square arrays only, for the reason ``vs_m`` gives."""
    import torch
    from . import angular, synth
    from .engine import randperm
    from .pipeline import infer_low_rank_pipeline_batch
    from .scan import beam_scan_batch
    from .solver import VARIANTS, synth_problem
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if tx != rx:
        raise ValueError(f"vs_m_baselines needs tx == rx (got {tx} x {rx}): the synth's vec(H) order has rx leading")
    count, first, chunk = int(count), int(first), int(chunk)
    if count < 1 or first < 0 or chunk < 1:
        raise ValueError("count and chunk must be >= 1 and first >= 0")
    Ms = [int(M) for M in M_list]
    dev = torch.device("cuda" if device is None else device)
    cfg = pipeline_cfg(VARIANTS[method])
    R = cfg.restarts
    kw = {} if maxiter is None else {"maxiter": int(maxiter)}
    metrics = np.empty((len(Ms), count, 4), np.float64)
    status = np.empty((len(Ms), count), np.uint32)
    base = {k: np.empty((len(Ms), count), np.float64) for k in BASELINES}
    end = first + count
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    Wq, Fq = up(angular.quantize_ps(angular.dictionary(rx)[0])), up(angular.quantize_ps(angular.dictionary(tx)[0]))

    def gain_at(H, W, F, p, q):
        """|w^H H f| / sqrt(tx rx) from the scan's power of the true H at pair (p, q) per realisation; 0 where p < 0."""
        pw = beam_scan_batch(H, W, F, 1, want_power=True).power
        ok = p >= 0
        g = pw[torch.arange(pw.shape[0], device=dev), p.long().clamp(min=0), q.long().clamp(min=0)].sqrt() / math.sqrt(tx * rx)
        return torch.where(ok, g, torch.zeros_like(g)), ok

    for k, M in enumerate(Ms):
        mt = math.floor(M * cfg.cc_frac)
        nb = max(1, int(round(math.sqrt(M))))
        Ws, Fs = up(angular.sweep_beams(rx, nb)[0]), up(angular.sweep_beams(tx, nb)[0])
        for c0 in range(first // chunk * chunk, end, chunk):
            A, B, _, H = synth_problem(seed, c0, chunk, M, tx, rx, L=L, snr_db=snr_db, device=dev)
            tr = np.stack([np.stack([randperm(seed, (c0 + b) * R + i, M, mt) for i in range(R)])
                           for b in range(chunk)])
            rec = infer_low_rank_pipeline_batch(A, B, tx, rx, tr, variant=method, restarts=R, **kw)
            ev = evaluate_batch(rec.X, H, tx, rx)
            pc = evaluate_batch(H, H, tx, rx)
            aod_e, aoa_e, _, pe, qe = angular.estimate_angles(rec.X, tx, rx)
            g_est, ok = gain_at(H, Wq, Fq, pe, qe)
            Hraw = up(np.stack([synth.channel(seed, c0 + b, tx, rx, L) for b in range(chunk)]))
            aod_s, aoa_s, ps, qs = angular.beam_sweep(Hraw, tx, rx, nb, nb, snr_db=snr_db, seed=seed, first=c0)
            g_sw, _ = gain_at(H, Ws, Fs, ps, qs)
            tru = [synth.paths(seed, c0 + b, L) for b in range(chunk)]
            aod_t, aoa_t = np.stack([t[0] for t in tru]), np.stack([t[1] for t in tru])
            err_e = angular.aoda_err(aod_e.cpu().numpy(), aoa_e.cpu().numpy(), aod_t, aoa_t)
            err_e[~ok.cpu().numpy()] = angular.SEARCH_DEG
            cols = {"gain_percsi_ana": pc.gain_ana.cpu().numpy(), "gain_percsi_dig": pc.gain_dig.cpu().numpy(),
                    "aoda_err_est": err_e, "gain_est_aoda": g_est.cpu().numpy(), "gain_sweep": g_sw.cpu().numpy(),
                    "aoda_err_sweep": angular.aoda_err(aod_s.cpu().numpy(), aoa_s.cpu().numpy(), aod_t, aoa_t)}
            lo, hi = max(first, c0), min(end, c0 + chunk)   # the rows of this chunk the call asked for
            rows = slice(lo - first, hi - first)
            metrics[k, rows] = ev.metrics[lo - c0:hi - c0].cpu().numpy()
            status[k, rows] = ev.status[lo - c0:hi - c0].cpu().numpy().view(np.uint32)
            for name, v in cols.items():
                base[name][k, rows] = v[lo - c0:hi - c0]
    return {"M": np.asarray(Ms, np.int64), "metrics": metrics, "status": status,
            "mean": metrics.mean(axis=1), "n_degenerate": ((status & ACE_ST_EVAL_DEGENERATE) != 0).sum(axis=1),
            "columns": METRICS, **base, "baseline_mean": {name: v.mean(axis=1) for name, v in base.items()}}


VS_SNR_ADMM = ("A2only", "A2nuclear")
VS_SNR_SPARSE = ("plomp", "plgamp", "perfect_cs", "noisy_cs")


def vs_snr(tx, rx, M, snr_list, count, *, methods=("A2only", "plomp", "plgamp", "perfect_cs", "noisy_cs"), L=1,
           rician_k=5, search_deg=40.0, on_grid=False, noise="combiner", seed, first=0, chunk=CHUNK, pl_maxits=4000,
           maxiter=None, device=None, columns="h") -> dict:
    """The reference's ``Vs_SNR`` loop (Numerical_Simulation/main_programs/Vs_SNR.m:100-108: one dominant path with
    ``rician_k`` NLOS paths at the 7 dB K-factor, a searching area of ``search_deg`` degrees, M x M directional beams)
    with every step on the GPU: per SNR and realisation the scenario generator (``scenario.scenario_batch``), the
    recoveries and ``evaluate_batch``.  Only metrics and status words leave the device.

    What each method sees:

      * the sparse methods (``plomp``, ``plgamp``, ``perfect_cs``, ``noisy_cs``: Method.PLOMP, PLGAMP, PerfectPhaseCS,
        NoisyPhaseCS) the Kronecker codebook ``angular.kron_codebook`` of M x M ``angular.sweep_beams`` over
        ``search_deg`` (Directional_Beam_Angular.m), Phi = A AD with ``sparse.dictionary_2d(..., search_deg=search_deg)``
        and the measurements at the reference's own scale with noise model ``noise``: "combiner" is the reference's
        W' * noiseMatrix, "iid" one draw per probe.  M^2 may not exceed the OMP kernel's row limit;
      * the ADMM methods (``A2only``, ``A2nuclear``) a random phase-code codebook of M^2 rows with iid noise and the
        normalised B (MyCPR.m hands them measurementMat_RB, and random beams have no combiner structure), through
        ``vs_m``'s pipeline and train partitions.

    Random numbers.  Realisation b of the call is realisation ``first + b`` of the sweep; its channel and its
    unit-variance draws (noise, phase noise, start) depend on (seed, first + b) alone, so every SNR point sees the same
    channel and the same noise direction scaled by its sigma.  This is common random numbers; it departs from the
    reference, which draws afresh at every point.  Chunks lie on ``vs_m``'s grid (realisation i belongs to chunk
    i // chunk), so a shard reproduces its rows of the full run bit for bit.

    Returns ``snr`` [nSNR], per method its four ``evaluate_batch`` columns [nSNR][count][4] (key = the method's name),
    ``status_<method>`` [nSNR][count], ``mean`` (per method [nSNR][4]), ``gain_percsi_ana`` [nSNR][count]
    (``evaluate_batch(H, H)`` on the channel at the reference's scale), ``mCS`` and ``columns``.

    ``columns="recovery"`` adds, for the sparse methods, the score Vs_SNR.m:192-194 gives them, ``Evaluation_Recovery``
    (``recovery_eval.evaluate_recovery_batch``): ``recovery_<method>`` [nSNR][count][15] (columns ``columns_recovery``),
    ``status_recovery_<method>`` and ``mean_recovery``, with the scenario's true angles and the two sweep patterns on
    the M x M directional beams (``angular.beam_sweep`` on independent noise draws).  Every other key and value is
    bit-identical to the default ``columns="h"``."""
    import torch
    from . import angular, sparse
    from .engine import randperm
    from .pipeline import infer_low_rank_pipeline_batch
    from .scenario import scenario_batch
    from ._lib import LIB, check, scenario_cfg
    from .solver import VARIANTS
    methods = tuple(methods)
    bad = [k for k in methods if k not in VS_SNR_ADMM + VS_SNR_SPARSE]
    if bad or not methods:
        raise ValueError(f"methods must come from {VS_SNR_ADMM + VS_SNR_SPARSE}, got {bad or methods}")
    if tx != rx:
        raise ValueError(f"vs_snr needs tx == rx (got {tx} x {rx}): the synth's vec(H) order has rx leading")
    if noise not in ("combiner", "iid"):
        raise ValueError(f"noise must be 'combiner' or 'iid', got {noise!r}")
    want_rec = _check_columns(columns)
    count, first, chunk, M = int(count), int(first), int(chunk), int(M)
    if count < 1 or first < 0 or chunk < 1 or M < 1:
        raise ValueError("count, chunk and M must be >= 1 and first >= 0")
    m = M * M
    sp = [k for k in methods if k in VS_SNR_SPARSE]
    ad = [k for k in methods if k in VS_SNR_ADMM]
    if sp and m > sparse.D_MAX:
        raise ValueError(f"vs_snr: M = {M} gives M^2 = {m} measurements > {sparse.D_MAX}, the OMP kernel's row limit "
                         f"(methods {sp})")
    snrs = [float(v) for v in snr_list]
    dev = torch.device("cuda" if device is None else device)
    n, s = tx * rx, int(L)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    base = dict(L=int(L), rician_k=int(rician_k), search_deg=float(search_deg), on_grid=int(bool(on_grid)))
    out = {k: np.empty((len(snrs), count, 4), np.float64) for k in methods}
    stat = {k: np.zeros((len(snrs), count), np.uint32) for k in methods}
    percsi = np.empty((len(snrs), count), np.float64)
    mcs = 0
    if sp:
        Ft, Wr = angular.sweep_beams(tx, M, search_deg)[0] / np.sqrt(tx), angular.sweep_beams(rx, M, search_deg)[0] / np.sqrt(rx)
        As, Wd = up(angular.kron_codebook(Ft, Wr)), up(Wr)
        AD = up(sparse.dictionary_2d(tx, rx, search_deg=search_deg)[0])
        Phi = (As @ AD).contiguous()
        setup = sparse.two_stage_setup(Phi.cpu().numpy(), s).to(dev)
        mcs = setup.mCS
    rec, rec_st = {}, {}
    if want_rec and sp:
        from . import recovery_eval
        rec = {k: np.empty((len(snrs), count, recovery_eval.NCOL), np.float64) for k in sp}
        rec_st = {k: np.zeros((len(snrs), count), np.uint32) for k in sp}
        tb = recovery_eval.recovery_tables(tx, rx, None, None, search_deg)
        sw = recovery_eval.sweep_tables(tx, rx, M, M, search_deg)
    if ad:
        Ar = torch.empty((1, m, n), dtype=torch.complex128, device=dev)
        check(LIB.ace_synth_codebook(seed, -1, 1, m, n, Ar.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        kw = {} if maxiter is None else {"maxiter": int(maxiter)}
    end = first + count
    for k, snr in enumerate(snrs):
        for c0 in range(first // chunk * chunk, end, chunk):
            lo, hi = max(first, c0), min(end, c0 + chunk)   # the rows of this chunk the call asked for
            rows, sel = slice(lo - first, hi - first), slice(lo - c0, hi - c0)
            res = {}
            if sp:
                cfg = scenario_cfg(snr_db=snr, noise_model=1 if noise == "combiner" else 0, **base)
                sc = scenario_batch(seed, c0, chunk, tx, rx, As, cfg, Wd if noise == "combiner" else None,
                                    want=("vecH", "y", "y_noisy", "B_raw") + (("paths",) if rec else ()))
                H = sc.vecH
                if "plomp" in sp or "plgamp" in sp:
                    ts, sig = sparse.plomp_stage1(Phi, sc.B_raw * sc.B_raw, s, setup=setup, maxIts=int(pl_maxits))
                    if "plomp" in sp:
                        res["plomp"] = (sparse.omp_batch(ts.C, sig, ts.mCS, 1e-12), H)
                    if "plgamp" in sp:
                        res["plgamp"] = (sparse._gamp_stage2(ts, sig, s, sc.noise_power, Phi.shape[1]), H)
                if "perfect_cs" in sp:
                    res["perfect_cs"] = (sparse.perfect_phase_cs(Phi, sc.y, s), H)
                if "noisy_cs" in sp:
                    res["noisy_cs"] = (sparse.noisy_phase_cs(Phi, sc.y_noisy, s), H)
            if ad:
                sa = scenario_batch(seed, c0, chunk, tx, rx, Ar, scenario_cfg(snr_db=snr, noise_model=0, **base),
                                    want=("vecH", "B", "Hn"))
                H = sa.vecH
                for name in ad:
                    pc = pipeline_cfg(VARIANTS[name])
                    R, mt = pc.restarts, math.floor(m * pc.cc_frac)
                    tr = np.stack([np.stack([randperm(seed, (c0 + b) * R + i, m, mt) for i in range(R)])
                                   for b in range(chunk)])
                    res[name] = (infer_low_rank_pipeline_batch(Ar, sa.B, tx, rx, tr, variant=name, restarts=R, **kw), sa.Hn)
            percsi[k, rows] = evaluate_batch(H, H, tx, rx).gain_ana[sel].cpu().numpy()
            for name, (r, G) in res.items():
                X = r.X if name in ad else r.channel(AD)
                ev = evaluate_batch(X, G, tx, rx)
                st = ev.status if name in ad else (ev.status | r.status)
                out[name][k, rows] = ev.metrics[sel].cpu().numpy()
                stat[name][k, rows] = st[sel].cpu().numpy().view(np.uint32)
            if rec:
                aod, aoa = recovery_eval.split_paths(sc.paths, int(L))
                aod, aoa = aod.contiguous(), aoa.contiguous()
                picks = _sweep_picks(sc.vecH, tx, rx, M, M, snr, seed, c0, search_deg)
                for name in sp:
                    r = res[name][0]
                    rv = recovery_eval.evaluate_recovery_batch(_dense_z(r), sc.vecH, aod, aoa, tb,
                                                               noise_power=sc.noise_power, picks=picks, sweep=sw)
                    rec[name][k, rows] = rv.metrics[sel].cpu().numpy()
                    rec_st[name][k, rows] = (rv.status[sel] | r.status[sel]).cpu().numpy().view(np.uint32)
    return {"snr": np.asarray(snrs, np.float64), "M": M, "mCS": mcs, "s": s, **out, "columns": METRICS,
            "gain_percsi_ana": percsi, **{f"status_{k}": v for k, v in stat.items()},
            "mean": {k: v.mean(axis=1) for k, v in out.items()}, **_recovery_keys(rec, rec_st)}


# the table of VS_SR_par.m:74-99: searching area -> (M, G) pairs
VS_SR_AREAS = (20, 30, 40, 50, 60, 70, 80)
VS_SR_M = ((2, 3, 4, 5), (4, 5, 6, 7), (5, 6, 7, 8, 9), (6, 7, 8, 9, 10, 11), (8, 9, 10, 11, 12), (9, 10, 11, 12, 13),
           (10, 11, 12, 13, 14))
VS_SR_G = ((25, 35, 45, 55), (25, 40, 55, 60), (25, 40, 55, 60, 70), (25, 40, 45, 55, 65, 70), (40, 50, 55, 60, 70),
           (40, 55, 60, 70, 75), (45, 55, 60, 70, 75))
VS_SR_MAEE = (0.6, 0.8, 1.0)   # VS_SR_par.m:105
VS_SR_ANTENNAS = 12            # sub_VS_SR_par.m:56-57


def vs_sr(tx=VS_SR_ANTENNAS, rx=VS_SR_ANTENNAS, area_list=VS_SR_AREAS, M_lists=VS_SR_M, G_lists=VS_SR_G, count=100, *,
          methods=("plomp", "plgamp", "perfect_cs", "noisy_cs"), snr_db=0.0, rician_k=5, seed, first=0, chunk=CHUNK,
          noise="combiner", pl_maxits=4000, maee_set=VS_SR_MAEE, return_inputs=False, device=None) -> dict:
    """The reference's ``VS_SR_par.m`` / ``sub_VS_SR_par.m``: how side information (a narrower searching area) reduces
    the training overhead.  Per searching area ``area_list[a]`` (degrees) and per pair ``(M_lists[a][i], G_lists[a][i])``:
    one dominant path (L = 1) at off-grid angles inside the area with ``rician_k`` NLOS paths
    (``scenario.scenario_batch``), M x M ``angular.directional_beams`` probes over the area (Directional_Beam_Angular),
    the dictionary on a grid of NQ = G points per side cut to the area, the two-stage recoveries (``plomp``, ``plgamp``)
    and the conventional-CS benchmarks (``perfect_cs``, ``noisy_cs``) of ``vs_snr``, and the reference's own score,
    ``Evaluation_Recovery`` (``recovery_eval.evaluate_recovery_batch``), with the two sweep patterns on the same beams.
    Every step runs on the GPU; only metrics and status words leave the device.  The defaults are the reference's:
    12 x 12 antennas (sub_VS_SR_par.m:56-57), SNR 0 dB, the table of VS_SR_par.m:74-99.

    Random numbers are ``vs_snr``'s: realisation b of the call is realisation ``first + b`` of the sweep, its draws
    depend on (seed, first + b) alone (common random numbers across the sweep points, where the reference draws afresh),
    and chunks lie on the grid of the realisation index, so shards compose.

    Returns ``area`` [nArea], ``M`` and ``G`` [nArea][nM] (nM the longest list; -1 pads the shorter ones), ``nM``
    [nArea], per method its 15 columns [nArea][nM][count][15] (key = the method's name, columns ``columns`` =
    ``recovery_eval.METRICS_RECOVERY``, NaN in the padding), ``status_<method>`` [nArea][nM][count] (the evaluator's bits
    or-ed with the solver's), ``mean`` (per method [nArea][nM][15]), ``mCS`` [nArea][nM], and the read-out of
    VS_SR_par.m:105-125: ``M_at_maee`` (per method [nArea][len(maee_set)]), the M at which the method's mean AoDA_Err
    (column 1, the MAEE) comes nearest to each value of ``maee_set``, the first on a tie; the reference plots its square.
    ``return_inputs=True`` also copies each point's channels, paths, picks and recovered vectors to the host
    (``inputs[a][i]``: a dict), for tests and diagnosis."""
    import torch
    from . import angular, recovery_eval, sparse
    from .scenario import scenario_batch
    from ._lib import scenario_cfg
    methods = tuple(methods)
    bad = [k for k in methods if k not in VS_SNR_SPARSE]
    if bad or not methods:
        raise ValueError(f"methods must come from {VS_SNR_SPARSE}, got {bad or methods}")
    if tx != rx:
        raise ValueError(f"vs_sr needs tx == rx (got {tx} x {rx}): the sparse recoveries it shares with vs_snr are square-only")
    if noise not in ("combiner", "iid"):
        raise ValueError(f"noise must be 'combiner' or 'iid', got {noise!r}")
    areas = [float(a) for a in area_list]
    Ml, Gl = [[int(v) for v in r] for r in M_lists], [[int(v) for v in r] for r in G_lists]
    if len(Ml) != len(areas) or len(Gl) != len(areas) or any(len(a) != len(b) or not a for a, b in zip(Ml, Gl)):
        raise ValueError("M_lists and G_lists need one list per searching area, of equal non-zero lengths")
    count, first, chunk = int(count), int(first), int(chunk)
    if count < 1 or first < 0 or chunk < 1:
        raise ValueError("count and chunk must be >= 1 and first >= 0")
    if any(M < 1 or M * M > sparse.D_MAX for r in Ml for M in r):
        raise ValueError(f"vs_sr: M^2 measurements must be 1..{sparse.D_MAX}, the OMP kernel's row limit")
    if any(G < 1 for r in Gl for G in r):
        raise ValueError("vs_sr: the grid sizes must be >= 1")
    dev = torch.device("cuda" if device is None else device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    nA, nM, NC = len(areas), max(len(r) for r in Ml), recovery_eval.NCOL
    out = {k: np.full((nA, nM, count, NC), np.nan) for k in methods}
    stat = {k: np.zeros((nA, nM, count), np.uint32) for k in methods}
    Mpad, Gpad, mcs = np.full((nA, nM), -1, np.int64), np.full((nA, nM), -1, np.int64), np.full((nA, nM), -1, np.int64)
    inputs = [[None] * len(r) for r in Ml]
    end, s = first + count, 1
    for a, area in enumerate(areas):
        for i, (M, G) in enumerate(zip(Ml[a], Gl[a])):
            Mpad[a, i], Gpad[a, i] = M, G
            Ft, Wr = angular.directional_beams(tx, M, area)[0] / np.sqrt(tx), angular.directional_beams(rx, M, area)[0] / np.sqrt(rx)
            As, Wd = up(angular.kron_codebook(Ft, Wr)), up(Wr)
            Phi = (As @ up(sparse.dictionary_2d(tx, rx, G, G, search_deg=area)[0])).contiguous()
            tb = recovery_eval.recovery_tables(tx, rx, G, G, area)
            sw = recovery_eval.sweep_tables(tx, rx, M, M, area)
            setup = None
            if "plomp" in methods or "plgamp" in methods:
                setup = sparse.two_stage_setup(Phi.cpu().numpy(), s).to(dev)
                mcs[a, i] = setup.mCS
            cfg = scenario_cfg(L=1, rician_k=int(rician_k), search_deg=area, on_grid=0, NQt=G, NQr=G, snr_db=float(snr_db),
                               noise_model=1 if noise == "combiner" else 0)
            keep = {} if not return_inputs else {"vecH": [], "paths": [], "picks": [], **{f"z_{k}": [] for k in methods}}
            for c0 in range(first // chunk * chunk, end, chunk):
                lo, hi = max(first, c0), min(end, c0 + chunk)   # the rows of this chunk the call asked for
                rows, sel = slice(lo - first, hi - first), slice(lo - c0, hi - c0)
                sc = scenario_batch(seed, c0, chunk, tx, rx, As, cfg, Wd if noise == "combiner" else None,
                                    want=("vecH", "y", "y_noisy", "B_raw", "paths"))
                res = {}
                if setup is not None:
                    ts, sig = sparse.plomp_stage1(Phi, sc.B_raw * sc.B_raw, s, setup=setup, maxIts=int(pl_maxits))
                    if "plomp" in methods:
                        res["plomp"] = sparse.omp_batch(ts.C, sig, ts.mCS, 1e-12)
                    if "plgamp" in methods:
                        res["plgamp"] = sparse._gamp_stage2(ts, sig, s, sc.noise_power, Phi.shape[1])
                if "perfect_cs" in methods:
                    res["perfect_cs"] = sparse.perfect_phase_cs(Phi, sc.y, s)
                if "noisy_cs" in methods:
                    res["noisy_cs"] = sparse.noisy_phase_cs(Phi, sc.y_noisy, s)
                aod, aoa = recovery_eval.split_paths(sc.paths, 1)
                aod, aoa = aod.contiguous(), aoa.contiguous()
                picks = _sweep_picks(sc.vecH, tx, rx, M, M, float(snr_db), seed, c0, area)
                if return_inputs:
                    keep["vecH"].append(sc.vecH[sel].cpu().numpy())
                    keep["paths"].append(sc.paths[sel].cpu().numpy())
                    keep["picks"].append(picks[sel].cpu().numpy())
                for name, r in res.items():
                    z = _dense_z(r)
                    rv = recovery_eval.evaluate_recovery_batch(z, sc.vecH, aod, aoa, tb, noise_power=sc.noise_power,
                                                               picks=picks, sweep=sw)
                    out[name][a, i, rows] = rv.metrics[sel].cpu().numpy()
                    stat[name][a, i, rows] = (rv.status[sel] | r.status[sel]).cpu().numpy().view(np.uint32)
                    if return_inputs:
                        keep[f"z_{name}"].append(z[sel].cpu().numpy())
            if return_inputs:
                inputs[a][i] = {**{k: np.concatenate(v) for k, v in keep.items()}, "noise_power": sc.noise_power,
                                "tables": tb, "sweep": sw}
    mean = {k: v.mean(axis=2) for k, v in out.items()}
    at = {}
    for k in methods:
        at[k] = np.full((nA, len(maee_set)), -1, np.int64)
        for a in range(nA):
            maee = mean[k][a, :len(Ml[a]), 1]
            for j, target in enumerate(maee_set):
                at[k][a, j] = Ml[a][int(np.argmin(np.abs(maee - float(target))))]   # (:115-118: min takes the first)
    ret = {"area": np.asarray(areas, np.float64), "M": Mpad, "G": Gpad, "nM": np.asarray([len(r) for r in Ml], np.int64),
           **out, "columns": recovery_eval.METRICS_RECOVERY, **{f"status_{k}": v for k, v in stat.items()}, "mean": mean,
           "mCS": mcs, "M_at_maee": at, "maee_set": tuple(float(v) for v in maee_set)}
    if return_inputs:
        ret["inputs"] = inputs
    return ret
