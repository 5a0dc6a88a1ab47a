"""GPU tests of the real-trace sweep and tracker (ace_amd.realtrace: VS_M_real_rss.m and the loop of
RSS_Mobility_simu.m:131-165, scored by Evaluate_rss on held-out probes).

The traces are synthetic: channels from ace_amd.synth measured through the committed reference codebook (a
512-row slice of tests/golden/ref_codebooks_16x16_packed.npz, ``random``) or, for the tracker, an 8 x 8 phase-code
codebook, with 1 % multiplicative noise, stored in dBm as a testbed would.  Every stage is capped with
``maxiter`` so that a test takes seconds; no accuracy is asserted for the recovered channels (DESIGN.md §4d has
the measured table): the tests pin what the functions compute -- the composition written out by hand, bit for
bit -- and the metric against tests/rss_ref.py inside its derived tolerance.
"""
import functools
import math
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import rss_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, MAXITER, N_TEST, M_LIST = 2024, 25, 112, [64, 256]


def _to_dbm(amp):
    from ace_amd import engine
    return 10.0 * np.log10(1000.0 * (amp / engine.RSS_FCT) ** 2)


@functools.lru_cache(maxsize=None)
def _trace16():
    """(cb [512][256], rss_dbm [4][512]): T = 4 channels through the reference codebook's first 512 rows."""
    from conftest import ROOT
    from ace_amd import synth
    p = np.load(ROOT / "tests" / "golden" / "ref_codebooks_16x16_packed.npz")["random"][:512]
    k = np.stack([(p >> (2 * i)) & 3 for i in range(4)], axis=-1).reshape(p.shape[0], -1).astype(np.int64)
    cb = (1j ** k).astype(np.complex128)          # exact +-1, +-j as main.py hands them to the driver
    H = np.stack([synth.channel(SEED, t, 16, 16) for t in range(4)])
    rng = np.random.default_rng(SEED)
    amp = np.abs(H @ cb.T) * (1 + 0.01 * rng.standard_normal((4, 512))) * 40.0
    dbm = _to_dbm(np.abs(amp))
    cb.setflags(write=False)
    dbm.setflags(write=False)
    return cb, dbm


@functools.lru_cache(maxsize=None)
def _full_run():
    from ace_amd import realtrace
    cb, dbm = _trace16()
    return realtrace.vs_m(cb, dbm, 16, 16, M_LIST, n_test=N_TEST, method="A2only", seed=SEED, maxiter=MAXITER,
                          chunk=2, return_X=True)


def test_vs_m_equals_the_composition_by_hand(gpu):
    import torch
    from ace_amd import dbm_to_amp, engine, evaluate_rss_batch, infer_low_rank_pipeline_batch, pipeline_cfg
    cb, dbm = _trace16()
    out = _full_run()
    assert out["M"].tolist() == M_LIST and out["metrics"].shape == (2, 4, 4) and out["status"].shape == (2, 4)
    assert out["test_rows"].tolist() == list(range(400, 512))
    assert np.array_equal(out["mean"], out["metrics"].mean(axis=1)) and np.isfinite(out["metrics"]).all()
    cfg = pipeline_cfg(0)
    R = cfg.restarts
    cbd = torch.from_numpy(np.array(cb)).to(gpu)      # (copies: the shared inputs are read-only)
    amp = dbm_to_amp(torch.from_numpy(np.array(dbm)).to(gpu))
    test = torch.arange(400, 512, device=gpu)
    for k, M in enumerate(M_LIST):
        rows = out["rows"][k]
        assert rows.tolist() == list(range(M))          # rows="first": picked_beams = 1:M
        ridx = torch.as_tensor(rows, device=gpu)
        mt = math.floor(M * cfg.cc_frac)
        for c0 in (0, 2):
            tr = np.stack([np.stack([engine.randperm(SEED, t * R + i, M, mt) for i in range(R)])
                           for t in range(c0, c0 + 2)])
            rec = infer_low_rank_pipeline_batch(cbd[ridx].contiguous(), amp[c0:c0 + 2][:, ridx].contiguous(), 16, 16,
                                                tr, variant="A2only", restarts=R, maxiter=MAXITER)
            ev = evaluate_rss_batch(rec.X, cbd[test].contiguous(), amp[c0:c0 + 2][:, test].contiguous())
            assert np.array_equal(ev.metrics.cpu().numpy(), out["metrics"][k, c0:c0 + 2]), (M, c0)
            assert np.array_equal(ev.status.cpu().numpy().view(np.uint32), out["status"][k, c0:c0 + 2])
            assert torch.equal(rec.X, out["X"][k, c0:c0 + 2])


def test_vs_m_metrics_agree_with_the_exact_reference_on_the_returned_estimates(gpu):
    from ace_amd import dbm_to_amp
    cb, dbm = _trace16()
    out = _full_run()
    amp = dbm_to_amp(dbm)
    for k in range(len(M_LIST)):
        X = out["X"][k].cpu().numpy()
        assert np.isfinite(X.view(np.float64)).all()
        ref = RR.exact(X, cb[400:], amp[:, 400:])
        assert np.array_equal(out["status"][k], ref["status"])
        assert np.array_equal(out["metrics"][k][:, 3], ref["metrics"][:, 3].astype(np.float64))
        q = RR.ratios(out["metrics"][k], None, ref)
        print(f"M = {M_LIST[k]}: mean_rel {out['metrics'][k][:, 0]}, worst err/tol {q}")
        assert max(q.values()) <= 1.0, q


def test_vs_m_subset_of_the_traces_reproduces_its_rows(gpu):
    from ace_amd import realtrace
    cb, dbm = _trace16()
    full = _full_run()
    sub = realtrace.vs_m(cb, dbm[2:4], 16, 16, M_LIST[:1], n_test=N_TEST, seed=SEED, maxiter=MAXITER, chunk=2, first=2)
    assert np.array_equal(sub["metrics"][0], full["metrics"][0, 2:4])
    assert np.array_equal(sub["status"][0], full["status"][0, 2:4])
    with pytest.raises(ValueError):
        realtrace.vs_m(cb, dbm[1:3], 16, 16, M_LIST[:1], n_test=N_TEST, seed=SEED, chunk=2, first=1)


def test_vs_m_randperm_rows_and_explicit_test_rows(gpu):
    from ace_amd import engine, realtrace
    cb, dbm = _trace16()
    test_rows = np.arange(5, 512, 5)[:100]
    out = realtrace.vs_m(cb, dbm[0], 16, 16, [64, 96], test_rows=test_rows, rows="randperm", seed=SEED,
                         maxiter=MAXITER)
    pool = np.setdiff1d(np.arange(512), test_rows)
    for k, M in enumerate([64, 96]):
        assert out["rows"][k].tolist() == pool[engine.randperm(SEED, k, pool.size, M)].tolist()
        assert not set(out["rows"][k].tolist()) & set(test_rows.tolist())
    assert out["metrics"].shape == (2, 1, 4) and (out["metrics"][:, 0, 3] == 100).all()
    with pytest.raises(ValueError):
        realtrace.vs_m(cb, dbm, 16, 16, [64], seed=SEED)                               # neither test_rows nor n_test
    with pytest.raises(ValueError):
        realtrace.vs_m(cb, dbm, 16, 16, [64], n_test=N_TEST, method="phaselift", seed=SEED)


# ---------------------------------------------------------------- the tracker, 8 x 8
SLOT, M_MAX, KEEP = 32, 24, 60


@functools.lru_cache(maxsize=None)
def _trace8():
    """(cb [384][64], rss_dbm [384]): 12 slots of 32 probes of one 8 x 8 channel in time order."""
    from ace_amd import synth
    cb = synth.codebook(SEED, 12 * SLOT, 64)
    h = synth.channel(SEED, 7, 8, 8)
    rng = np.random.default_rng(SEED + 1)
    amp = np.abs(cb @ h) * (1 + 0.01 * rng.standard_normal(12 * SLOT)) * 40.0
    return cb, _to_dbm(np.abs(amp))


def test_track_follows_the_rule_and_equals_the_composition_by_hand(gpu):
    import torch
    from ace_amd import dbm_to_amp, engine, evaluate_rss_batch, infer_low_rank_pipeline_batch, pipeline_cfg, realtrace
    cb, dbm = _trace8()
    cb, dbm = cb[:6 * SLOT], dbm[:6 * SLOT]
    out = realtrace.track(cb, dbm, 8, 8, slot=SLOT, m_max=M_MAX, keep=KEEP, seed=SEED, maxiter=MAXITER)
    M, score = out["M"], out["mean_rel"]
    assert M.shape == (6,) and M[0] == M_MAX and np.isfinite(score).all() and (score > 0).all()
    for t in range(5):
        assert M[t + 1] == realtrace.next_m(M[t], score[t], M_MAX, 0.2), t
    cfg = pipeline_cfg(0)
    R = cfg.restarts
    cbd = torch.from_numpy(cb).to(gpu)
    amp = dbm_to_amp(torch.from_numpy(dbm).to(gpu))
    window = np.zeros(0, np.int64)
    for t in range(6):
        window = np.concatenate([window, SLOT * t + np.arange(M[t])])[-(KEEP + 1):]
        assert window.size >= 22
        W = window.size
        tr = np.stack([engine.randperm(SEED, t * R + i, W, math.floor(W * cfg.cc_frac)) for i in range(R)])
        widx = torch.as_tensor(window, device=gpu)
        rec = infer_low_rank_pipeline_batch(cbd[widx].contiguous(), amp[widx][None].contiguous(), 8, 8, tr,
                                            variant="A2only", restarts=R, maxiter=MAXITER)
        ev = evaluate_rss_batch(rec.X, cbd[SLOT * t + M[t]:SLOT * (t + 1)], amp[SLOT * t + M[t]:SLOT * (t + 1)])
        assert float(ev.mean_rel[0]) == score[t], t
        assert int(ev.n_used[0]) == SLOT - M[t]
        assert np.uint32(int(ev.status[0])) == out["status"][t]


def test_track_with_an_infinite_threshold_walks_down_to_zero(gpu):
    from ace_amd import realtrace
    cb, dbm = _trace8()
    out = realtrace.track(cb, dbm, 8, 8, slot=SLOT, m_max=M_MAX, keep=KEEP, threshold=float("inf"), seed=SEED,
                          maxiter=MAXITER)
    assert out["M"].tolist() == [24, 19, 15, 11, 8, 6, 4, 3, 2, 1, 0, 0]
    assert np.isfinite(out["mean_rel"]).all()     # M = 0: nothing appended, the whole slot is the test set


def test_track_slot_without_test_rows_keeps_m_and_records_nan(gpu):
    from ace_amd import realtrace
    cb, dbm = _trace8()
    out = realtrace.track(cb[:2 * SLOT], dbm[:2 * SLOT], 8, 8, slot=SLOT, m_max=SLOT, seed=SEED, maxiter=MAXITER)
    assert out["M"].tolist() == [SLOT, SLOT] and np.isnan(out["mean_rel"]).all() and (out["status"] == 0).all()
    with pytest.raises(ValueError):
        realtrace.track(cb[:50], dbm[:50], 8, 8, slot=SLOT, seed=SEED)     # P no multiple of slot
