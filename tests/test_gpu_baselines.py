"""GPU tests of the angle estimates and the beam-sweep baseline (ace_amd.angular) and of the Monte-Carlo sweep with
its yardsticks (ace_amd.montecarlo.vs_m_baselines), against the same steps written out by hand with the exact
reference of tests/scan_ref.py.  Indices and angles are compared exactly (the precondition, separated leaders, is
asserted on the inputs); gains inside the scan's tolerance.  No recovery-quality threshold is asserted."""
import math
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import scan_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

N = 16
SEED, MAXITER, CHUNK, MS = 7, 60, 8, [121, 225]


def _true_channels(count, L=3, seed=1):
    from ace_amd import synth
    return np.stack([synth.channel(seed, b, N, N, L) for b in range(count)])


def test_estimate_angles_against_the_hand_composition(gpu):
    import torch
    from ace_amd import angular
    H = _true_channels(12)
    Ft, _, deg_t = angular.dictionary(N)
    Wr, _, deg_r = angular.dictionary(N)
    ref = SR.exact(H, Wr, Ft, 1)
    assert SR.gaps(ref, 1) > 1e-9
    f = ref["top_idx"][:, 0].astype(np.int64)
    p, q = f // Wr.shape[0], f % Wr.shape[0]
    for X in (torch.from_numpy(H).to(gpu), H):     # the device and the host entry
        aod, aoa, pw, pe, qe = (np.asarray(v.cpu() if hasattr(v, "cpu") else v) for v in angular.estimate_angles(X, N, N))
        assert np.array_equal(pe, p) and np.array_equal(qe, q)
        assert np.array_equal(aod, deg_t[p]) and np.array_equal(aoa, deg_r[q])     # bit for bit
        assert SR.ratios(ref, top_pow=pw[:, None])["top_pow"] <= 1.0


def test_beam_sweep_against_the_hand_composition(gpu):
    import torch
    from ace_amd import angular, synth
    H = _true_channels(12)
    Mt = Mr = 11
    snr, first = 10.0, 3
    # by hand: MyBeamSweeping.m:93-109, the synth's iid noise per pair from stream kind 8 of realisation first + b
    part = np.linspace(-47.5, 47.5, Mt + 1)
    cen = (part[:-1] + part[1:]) / 2
    ideal = np.exp(-1j * 2 * np.pi * synth.ANT_D / synth.LAMBDA * np.sin(np.deg2rad(cen))[:, None] * np.arange(N))
    B = angular.quantize_ps(ideal) / np.sqrt(N)
    noise = np.stack([synth.normal_pairs(SEED, synth.stream_id(8, first + b), Mt * Mr) for b in range(12)]) \
        * np.sqrt(0.5 * 10.0 ** (-snr / 10.0))
    ref = SR.exact(H, B, B, 1, noise)
    assert SR.gaps(ref, 1) > 1e-9
    f = ref["top_idx"][:, 0].astype(np.int64)
    p, q = f // Mr, f % Mr
    for X in (torch.from_numpy(H).to(gpu), H):
        aod, aoa, ps, qs = (np.asarray(v.cpu() if hasattr(v, "cpu") else v)
                            for v in angular.beam_sweep(X, N, N, Mt, Mr, snr_db=snr, seed=SEED, first=first))
        assert np.array_equal(ps, p) and np.array_equal(qs, q)
        assert np.array_equal(aod, cen[p]) and np.array_equal(aoa, cen[q])
    # a realisation's sweep depends on (seed, index) alone: realisations 5 .. 8 of the same sweep on their own
    sub = angular.beam_sweep(H[2:6], N, N, Mt, Mr, snr_db=snr, seed=SEED, first=first + 2)
    assert np.array_equal(sub[2], p[2:6]) and np.array_equal(sub[3], q[2:6])


@pytest.fixture(scope="module")
def sweeps(gpu):
    from ace_amd.montecarlo import vs_m, vs_m_baselines
    kw = dict(method="A2only", maxiter=MAXITER, seed=SEED, chunk=CHUNK)
    return {"plain": vs_m(N, N, MS, count=8, **kw), "base": vs_m_baselines(N, N, MS, count=8, **kw),
            "full": vs_m_baselines(N, N, MS, count=16, **kw), "shard": vs_m_baselines(N, N, MS, count=8, first=8, **kw)}


def test_vs_m_baselines_keeps_vs_m_and_composes(sweeps):
    from ace_amd.montecarlo import BASELINES
    plain, base, full, shard = (sweeps[k] for k in ("plain", "base", "full", "shard"))
    for k in ("M", "metrics", "status", "mean", "n_degenerate"):
        assert np.array_equal(base[k], plain[k]), k
    assert base["columns"] == plain["columns"]
    for name in BASELINES:
        assert base[name].shape == (2, 8) and np.isfinite(base[name]).all(), name
        assert np.array_equal(shard[name], full[name][:, 8:]), name
        assert np.array_equal(base[name], full[name][:, :8]), name
        assert np.array_equal(full["baseline_mean"][name], full[name].mean(axis=1))
    assert np.array_equal(shard["metrics"], full["metrics"][:, 8:]) and np.array_equal(shard["status"], full["status"][:, 8:])


def test_vs_m_baselines_against_the_hand_composition(gpu, sweeps):
    from ace_amd import (angular, evaluate_batch, infer_low_rank_pipeline_batch, pipeline_cfg, synth, synth_problem)
    from ace_amd.engine import randperm
    from ace_amd.solver import VARIANTS
    base = sweeps["base"]
    cfg = pipeline_cfg(VARIANTS["A2only"])
    R = cfg.restarts
    Ft, _, deg = angular.dictionary(N)
    Q = Ft.shape[0]
    Fq = angular.quantize_ps(Ft)
    tru = [synth.paths(SEED, b, 3) for b in range(CHUNK)]
    aod_t, aoa_t = np.stack([t[0] for t in tru]), np.stack([t[1] for t in tru])
    Hraw = np.stack([synth.channel(SEED, b, N, N, 3) for b in range(CHUNK)])
    for k, M in enumerate(MS):
        mt = math.floor(M * cfg.cc_frac)
        A, B, _, H = synth_problem(SEED, 0, CHUNK, M, N, N, L=3, snr_db=30.0, device=gpu)
        tr = np.stack([np.stack([randperm(SEED, b * R + i, M, mt) for i in range(R)]) for b in range(CHUNK)])
        rec = infer_low_rank_pipeline_batch(A, B, N, N, tr, variant="A2only", restarts=R, maxiter=MAXITER)
        pc = evaluate_batch(H, H, N, N)
        assert np.array_equal(base["gain_percsi_ana"][k], pc.gain_ana.cpu().numpy())
        assert np.array_equal(base["gain_percsi_dig"][k], pc.gain_dig.cpu().numpy())
        Xh, Hh = rec.X.cpu().numpy(), H.cpu().numpy()
        assert np.isfinite(Xh).all()
        # the estimate's angles: the exact scan of the recovered channel with the two dictionaries
        est = SR.exact(Xh, Ft, Ft, 1)
        assert SR.gaps(est, 1) > 1e-9
        f = est["top_idx"][:, 0].astype(np.int64)
        p, q = f // Q, f % Q
        assert np.array_equal(base["aoda_err_est"][k], angular.aoda_err(deg[p], deg[q], aod_t, aoa_t))
        # the gain of the quantised steering pair on the true H, inside the scan's tolerance
        tmap = SR.exact(Hh, Fq, Fq, 1)
        rows = np.arange(CHUNK)

        def gain_ok(got, ref, ff):
            want, tol = ref["power"][rows, ff].astype(np.float64), ref["tol_power"][rows, ff]
            g2 = (got * N) ** 2            # the gains carry Quantize_PS's 1 / sqrt(tx rx), as gain_ana does
            return np.all(np.abs(g2 - want) <= tol + 8 * SR.U * want)    # (the square root, the division, the square)

        assert gain_ok(base["gain_est_aoda"][k], tmap, f)
        # the sweep: round(sqrt(M)) beams per side on the channel at the synth's scale, gain on the true H
        nb = round(math.sqrt(M))
        Bs, cen = angular.sweep_beams(N, nb)
        sw = SR.exact(Hraw, Bs / np.sqrt(N), Bs / np.sqrt(N), 1, angular.sweep_noise(SEED, 0, CHUNK, nb, nb, 30.0))
        assert SR.gaps(sw, 1) > 1e-9
        fs = sw["top_idx"][:, 0].astype(np.int64)
        assert np.array_equal(base["aoda_err_sweep"][k], angular.aoda_err(cen[fs // nb], cen[fs % nb], aod_t, aoa_t))
        assert gain_ok(base["gain_sweep"][k], SR.exact(Hh, Bs, Bs, 1), fs)
        # what holds in exact arithmetic, asserted with the scan's tolerance of y for unit-norm beams (S <= sum |H_ij|):
        # no unit-norm beam pair beats the channel's own singular pair
        slack = SR.C_Y * (2 * N + 8) * SR.U * np.abs(Hh).sum(axis=1)
        dig = base["gain_percsi_dig"][k]
        assert np.all(dig >= base["metrics"][k][:, 2] - slack)                  # gain_dig
        for name in ("gain_sweep", "gain_est_aoda", "gain_percsi_ana"):
            assert np.all(dig >= base[name][k] - slack), name
        assert np.all(dig >= base["metrics"][k][:, 1] - slack)                  # gain_ana
        print(f"M = {M}: gain_ana {base['metrics'][k][:, 1].mean():.3f} gain_sweep {base['gain_sweep'][k].mean():.3f} "
              f"gain_est_aoda {base['gain_est_aoda'][k].mean():.3f} percsi_ana {base['gain_percsi_ana'][k].mean():.3f}; "
              f"aoda_err est {base['aoda_err_est'][k].mean():.2f} sweep {base['aoda_err_sweep'][k].mean():.2f} deg")
