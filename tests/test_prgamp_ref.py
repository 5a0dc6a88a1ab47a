"""CPU tests of the PR-GAMP restatement (tests/prgamp_ref.py) and of the parity cases built on it.

For every realisation of every GPU parity case, each discrete decision the GPU comparison treats as exact (the pass
test against the window minimum, the GAMP tolerance test, estimInvert's loop conditions and its 1.01 NR0 retry test,
the EM stop, the misconvergence test, the best-residual update, the try stop) has a margin above 64 x the distance
between the f64 and the long-double run at that point, and the f64 run on permuted atoms takes the same decisions.
Seeds without that margin are passed over HERE (prgamp_ref.case walks a deterministic candidate stream), so that no
case and no realisation is excused at GPU time.

Sanity of the restatement: at (64, 48), 60 dB, with the full MyCPR option set it recovers x up to a global phase to
-40 dB.  The signal of that case has 4 active entries.  With a dense signal the same shape cannot converge: 64 real
magnitudes do not determine the 95 real unknowns of a 48-vector up to its phase.  Measured with the restatement on the
dense candidate 0 (f64): the tries end at residuals of -5.6, +0.4, +0.8 dB and then near 0 dB with the noise variance
learned up to the signal power and xhat near 0; all 100 tries run (ACE_ST_PRGAMP_MAXTRY), error 0 dB.  A dense
48-vector at m = 200 is recovered to -59 dB (test below), as is the 4-sparse one at m = 64 (-69 dB).

log I0e of the restatement (its own series and asymptotic expansion, in long double) is checked against mpmath.
"""
import pathlib
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import prgamp_ref as PR  # noqa: E402

IDS = [f"{s}-{h}" for s, h in PR.CASES]


@pytest.mark.parametrize("name,horizon", PR.CASES, ids=IDS)
def test_every_decision_of_every_realisation_has_its_margin(name, horizon):
    c = PR.case(name, horizon)
    _, m, N, batch = PR.SHAPES[name][:4]
    assert c["D"].shape == (m, N) and c["Y"].shape == (batch, m) and c["G"].shape == (batch, c["kw"]["max_try"], N)
    for b in range(batch):
        r64, rl, rp = c["ref64"][b], c["ref"][b], c["spread"][b][3]
        ok, worst = PR.decisions_agree(r64, rl, 64.0)
        okp, worstp = PR.decisions_agree(rp, rl, 64.0)
        kinds = sorted({k for k, _ in rl["decisions"]})
        print(f"{name} {horizon} b={b}: {len(rl['decisions'])} decisions ({' '.join(kinds)}), smallest margin / distance "
              f"{worst:.3g} (permuted atoms {worstp:.3g}), status {rl['status']}, counts {rl['counts'].tolist()}")
        assert ok and worst > 64.0, (b, worst)
        assert okp and worstp > 64.0, (b, worstp)
        for r in (r64, rp):
            assert r["status"] == rl["status"] and r["counts"].tolist() == rl["counts"].tolist(), b
            assert np.array_equal(r["trace"], rl["trace"]), b


def test_the_cases_exercise_the_paths():
    """Failed iterations (the pass test says no), estimInvert attempts that run to their iteration cap and ones that
    stop on either tolerance, calls that stop on the GAMP tolerance and on the iteration count, EM loops that stop on
    their tolerance and on nitEM, tries that stop on the residual and tries that run out."""
    seen = dict(failed_it=0, gtol=0, nit=0, em_tol=0, em_max=0, stop=0, maxtry=0, inv_cap=0, inv_tol=0)
    for name, horizon in PR.CASES:
        c = PR.case(name, horizon)
        nit, nem, _ = PR.HORIZONS[horizon]
        for r in c["ref64"]:
            tr = r["trace"]
            seen["failed_it"] += int((tr[..., 1] < tr[..., 0]).any())
            seen["nit"] += int((tr[..., 0] == nit).any())
            seen["gtol"] += int(((tr[..., 0] > 0) & (tr[..., 0] < nit)).any())
            seen["stop"] += r["status"] == 0
            seen["maxtry"] += r["status"] == PR.ST_MAXTRY
            if r["status"] in (0, PR.ST_MAXTRY):
                seen["em_max"] += int(r["counts"][2] == nem + 1)
                seen["em_tol"] += int(r["counts"][2] < nem + 1)
            d = r["decisions"]
            run = 0
            for k, q in d:
                if k == "inv2" and q > 0:
                    run += 1
                elif k == "invretry":
                    seen["inv_cap"] += run >= 25
                    seen["inv_tol"] += run < 25
                    run = 0
    print(seen)
    assert min(seen.values()) >= 1, seen


def test_the_restatement_recovers_x_to_minus_40_db():
    c = PR.case("sparse-64x48", "mycpr")
    assert c["kw"] == dict(gamp_nit=200, nit_em=50, max_try=100)
    for b, r in enumerate(c["ref"]):
        x = c["X"][b]
        xh = np.asarray(r["xhat"], np.complex128)
        ph = np.vdot(xh, x)
        ph /= abs(ph)
        err = 20 * np.log10(np.linalg.norm(xh * ph - x) / np.linalg.norm(x))
        print(f"sparse-64x48 b={b}: error {err:.1f} dB, residual {float(r['info'][0]):.1f} dB, counts {r['counts'].tolist()}")
        assert r["status"] == 0 and err <= -40.0, (b, err)
        assert r["counts"][3] == 4           # the posterior support count finds the 4 active entries


def test_a_dense_signal_is_recovered_where_it_is_determined():
    rng = np.random.default_rng(1)
    m, N = 200, 48
    D = PR.dictionary("gauss", m, N)
    x = (1 + rng.random(N)) * np.exp(2j * np.pi * rng.random(N))
    sig = D @ x
    y = np.abs(sig + np.sqrt(np.mean(np.abs(sig) ** 2) / 1e6) * PR._cn(rng, m))
    g = rng.standard_normal((10, N)) + 1j * rng.standard_normal((10, N))
    r = PR.prgamp(D, y, 1.0, g, max_try=10)
    ph = np.vdot(r["xhat"], x)
    ph /= abs(ph)
    err = 20 * np.log10(np.linalg.norm(r["xhat"] * ph - x) / np.linalg.norm(x))
    assert r["status"] == 0 and err <= -40.0, err


def test_the_failed_and_degenerate_statuses():
    c = PR.case("16x16", "handle")
    D, y, g = c["D"], c["Y"][0], c["G"][0]
    for bad in (np.zeros_like(y), y * 1e160):
        r = PR.prgamp(D, bad, c["lam"], g, **c["kw"])
        assert r["status"] == PR.ST_FAILED and not r["xhat"].any() and r["counts"].tolist() == [0, 0, 0, -1]
    y2 = y.copy()
    y2[3] = np.nan
    assert PR.prgamp(D, y2, c["lam"], g, **c["kw"])["status"] == PR.ST_DEGENERATE
    # a GAMP call limited to one iteration exports rhat = NaN: every try misconverges, estFin_best is still assigned
    # (the residual is finite), so the tries run out
    r = PR.prgamp(D, y, c["lam"], np.tile(g, (3, 1)), gamp_nit=1, nit_em=0, max_try=3)
    assert r["status"] == PR.ST_MAXTRY and r["counts"][0] == 3


def _want(x):
    """log(I0(x) exp(-x)) at 50 digits: mpmath's besseli up to 1e5, Hankel's expansion (12 terms: below 1e-60) beyond."""
    x = mp.mpf(x)
    if x < 1e5:
        return mp.log(mp.besseli(0, x)) - x
    s, term = mp.mpf(0), mp.mpf(1)
    for k in range(1, 13):
        term *= mp.mpf((2 * k - 1) ** 2) / (8 * k * x)
        s += term
    return mp.log1p(s) - mp.log(2 * mp.pi * x) / 2


def test_log_i0e_of_the_restatement_against_mpmath():
    mp.mp.dps = 50
    xs = np.array([0.0, 1e-300, 1e-12, 1e-6, 1e-3, 0.5, np.nextafter(1.0, 0), 1.0, 2.0, 7.5, 15.0, 24.0,
                   np.nextafter(PR.XC, 0), PR.XC, 26.0, 40.0, 1e2, 1e4, 1e8, 1e12, 1e300])
    for rt, tol in ((PR.LD, 4 * float(np.finfo(PR.LD).eps)), (np.float64, 16 * PR.U)):
        got = PR.log_i0e(xs.astype(rt), rt)
        for x, g in zip(xs, got):
            want = _want(float(x))
            err = abs(mp.mpf(float(np.float64(g))) + mp.mpf(float(g - rt(np.float64(g)))) - want)
            assert err <= tol * max(1.0, abs(float(want))), (rt, float(x), float(g), float(want))
    assert np.isnan(PR.log_i0e(np.array([np.nan]))[0]) and PR.log_i0e(np.array([np.inf]))[0] == -np.inf
