"""CPU tests of the EM-BG-GAMP restatement (tests/gamp_ref.py) and of the parity cases built on it: every
realisation of every GPU parity case meets the conditions under which a bit-different f64 evaluation takes the same
decisions; the accepted set of each option set exercises every stopping path; the restatement is permutation-
equivariant and recovers a well-conditioned noiseless sparse signal."""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import gamp_ref as GR  # noqa: E402


@pytest.mark.parametrize("name,optset,max_em", GR.CASES, ids=[f"{s}-{o}-em{m}" for s, o, m in GR.CASES])
def test_every_realisation_of_every_case_meets_the_conditions(name, optset, max_em):
    c = GR.case(name, optset, max_em)
    _, d, N, batch = GR.SHAPES[name][:4]
    assert c["D"].shape == (d, N) and c["Y"].shape == (batch, d)
    for b, r in enumerate(c["ref64"]):
        print(f"{name} {optset} em{max_em} b={b}: pass margin {r['pass']:.2e}, tolerance distance {r['tol']:.2e}, "
              f"floor distance 2^{r['floor']:.1f}, status {r['status']}, em_iters {r['em_iters']}")
        assert r["pass"] >= GR.PASS_MARGIN, (b, r["pass"])
        assert r["tol"] >= GR.TOL_MARGIN, (b, r["tol"])
        assert r["floor"] >= 1.0, (b, r["floor"])                       # no |svar|, rvar within a factor 2 of eps
        t = c["ref"][b]                                                    # the target run takes the same decisions
        assert (t["status"], t["em_iters"], t["trace"]) == (r["status"], r["em_iters"], r["trace"]), b
        assert c["spread"][b][2]["trace"] == r["trace"], b                # ... and so does the run on permuted atoms


@pytest.mark.parametrize("optset", list(GR.OPTION_SETS))
def test_the_accepted_set_exercises_every_path(optset):
    em_tol = nan_break = max_em = g_nit = g_tol = g_step = 0
    for name, o, m in GR.CASES:
        if o != optset:
            continue
        for r in GR.case(name, o, m)["ref64"]:
            em_tol += m == 200 and r["status"] == 0
            nan_break += bool(r["status"] & GR.ST_NANBREAK)
            max_em += m == 2 and bool(r["status"] & GR.ST_MAXEM)
            g_nit += "nit" in r["why"]
            g_tol += "tol" in r["why"]
            g_step += "step" in r["why"]
    print(optset, dict(em_tol=em_tol, nan_break=nan_break, max_em=max_em, g_nit=g_nit, g_tol=g_tol, g_step=g_step))
    assert min(em_tol, nan_break, max_em, g_nit, g_tol, g_step) >= 1


def test_the_failed_status_is_reachable_with_finite_input():
    """The reference's asserts, reached with finite y: y = 0 makes the initial phi 0, a y whose squared norm
    overflows makes psi Inf and phi NaN (CAwgnEstimIn's assert(var0 > 0)); a non-finite y is the degenerate bit."""
    c = GR.case("16x16", "plgamp", 200)
    D, y = c["D"], c["Y"][0]
    for bad in (np.zeros_like(y), y * 1e160):
        r = GR.embgamp(D, bad, c["snr"], c["lam"])
        assert r["status"] == GR.ST_FAILED and r["em_iters"] == 0 and not r["xhat"].any()
    y2 = y.copy()
    y2[3] = np.nan
    assert GR.embgamp(D, y2, c["snr"], c["lam"])["status"] == GR.ST_DEGENERATE
    # a GAMP call limited to one iteration can only make its forced pass: the NaN break in the first EM iteration,
    # where the reference's post-loop update reads an unassigned Shat
    r = GR.embgamp(D, y, c["snr"], c["lam"], nit=1)
    assert r["status"] == GR.ST_FAILED | GR.ST_NANBREAK and r["em_iters"] == 1


@pytest.mark.parametrize("optset", list(GR.OPTION_SETS))
def test_permuting_the_atoms_permutes_xhat(optset):
    c = GR.case("gauss-33x130", optset, 200)
    N = c["D"].shape[1]
    perm = np.random.default_rng(77).permutation(N)
    for b in range(4):
        r = c["ref64"][b]
        rp = GR.embgamp(c["D"][:, perm], c["Y"][b], c["snr"], c["lam"], **c["kw"])
        assert rp["trace"] == r["trace"] and rp["status"] == r["status"]
        assert np.linalg.norm(rp["xhat"] - r["xhat"][perm]) <= 1e-10 * np.linalg.norm(r["xhat"])
        assert np.allclose(rp["params"], r["params"], rtol=1e-10, atol=0)


@pytest.mark.parametrize("learn", [False, True])
def test_a_noiseless_sparse_signal_is_recovered(learn):
    rng = np.random.default_rng(12)
    d, N, s = 40, 100, 3
    D = GR.dictionary("gauss", d, N, seed=3)
    x = np.zeros(N, np.complex128)
    sup = rng.choice(N, s, replace=False)
    x[sup] = (1.0 + rng.random(s)) * np.exp(2j * np.pi * rng.random(s))
    # (SNRdB only initialises psi; at 10 dB the EM loop runs to its tolerance and learns psi down to nothing, while
    # from 30 dB on this damped GAMP makes one pass in its second call, leaves through the NaN break and stays 30 % off)
    r = GR.embgamp(D, D @ x, 10.0, s / N, learn_lambda=learn)
    assert r["status"] == 0
    assert np.linalg.norm(r["xhat"] - x) <= 1e-9 * np.linalg.norm(x)
    assert set(np.argsort(-np.abs(r["xhat"]))[:s].tolist()) == set(sup.tolist())
