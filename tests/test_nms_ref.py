"""CPU self-test of tests/nms_ref.py, the references of the m-space iteration suite (tests/test_gpu_nms.py).

- the longdouble specification agrees with an mpmath evaluation of the same recurrences (m <= 40) to 1e-17 kappa |value|
  (not 1e-17 of the value itself: an output that cancels is known only to kappa times the arithmetic's unit): the
  headroom of longdouble under the tolerance, which is TOL_MULT u kappa |value| >= 1e-15 kappa |value|;
- with the exact G, the specification chained 8 iterations from init equals the n-space truth to 1e-25 in mpmath, every
  output and every control decision: the algebra of DESIGN section 2.9;
- with G rounded to f64, the carried A E and ||E||^2 stay within the propagated ||(I + K) G - I|| ||T|| bound (printed);
- every input of the GPU suite shows the case it was built for, at least 1e-6 from a tie in every decision;
- ORACLE_RATIO and the chain deviations are measured and printed; every wrong-step model fails the GPU suite's own
  comparisons (nms_ref.compare_step) on an input of that suite: ten-fold outside a tolerance, or a decision flipped.
"""
import mpmath as mp
import numpy as np
import pytest

import nms_ref as R

VEC = ("Yn", "M", "En", "AEn", "W")
SCAL = ("obj2", "nAX2", "nY2", "nJM2", "dY2", "na", "naz", "nbeta", "nep2", "res_comb", "jn2", "dZ2", "nX2", "nZ2")


def _ratios(ref, other, keys=VEC + SCAL, rows=None):
    """max over the run realisations of |other - ref| / (u S) per output."""
    run = ref["mask"]["run"] if rows is None else rows
    out = {}
    for k in keys:
        s = np.asarray(ref["scale"][k], np.longdouble)
        err = np.abs(np.asarray(other["val"][k]).astype(np.clongdouble) - ref["val"][k])
        with np.errstate(all="ignore"):
            r = np.where(s > 0, err / (R.U * s), np.where(err > 0, np.inf, 0.0))
        r = r[run]
        r = r[~np.isnan(r)]
        out[k] = float(r.max()) if r.size else 0.0
    if ref["mask"]["pend_in"].any():
        for k in ("dAtY", "nAtY"):
            p = ref["mask"]["pend_in"]
            err = np.abs(np.asarray(other["state"][k]).astype(np.longdouble) - ref["state"][k])[p]
            out[k] = float(np.max(err / (R.U * np.asarray(ref["scale"][k], np.longdouble)[p])))
    return out


def _same_decisions(a, b):
    for k in a["mask"]:
        assert np.array_equal(a["mask"][k], b["mask"][k]), k
    for k in R.FLAGS:
        assert np.array_equal(a["flags"][k], b["flags"][k]), k
    assert a["done_count"] == b["done_count"]


@pytest.mark.parametrize("name", ["m1-n4-b1-k0", "m16-n16-b15-k1", "m31-n16-b16-k5", "m33-n16-b17-pending-bump",
                                  "m40-n16-b16-fixpoint"])
def test_longdouble_spec_matches_mpmath(name):
    mp.mp.dps = R.DPS
    inp = R.case(name)
    b = inp["Yo"].shape[0]
    pend = np.flatnonzero(inp["flags"][:, 3])[:2].tolist()
    sub = R.rows(inp, sorted(set([0, b // 2, b - 1] + pend)))
    ld, mpv = R.mspace_step(sub, R.LD), R.mspace_step(sub, R.MP)
    _same_decisions(ld, mpv)
    worst = 0.0
    for k in VEC + SCAL + ("pd_rc", "pd_dZ2", "pd_nZ2", "nopt_a"):
        ref = np.asarray(mpv["val"][k])
        got = np.asarray(ld["val"][k])
        s = R.MP.f64(mpv["scale"][k]).astype(np.float64)
        err = np.array([float(abs(x - y)) for x, y in zip(_mp_list(got), ref.ravel())])
        with np.errstate(all="ignore"):
            r = np.where(s.ravel() > 0, err / s.ravel(), 0.0)
        worst = max(worst, float(np.nanmax(r)) if r.size else 0.0)
    print(f"  {name}: longdouble against mpmath, worst err / (kappa |value|) = {worst:.3g}")
    assert worst <= 1e-17


def _mp_list(x):
    """A longdouble / clongdouble array as a flat list of mpmath numbers, exactly (hi + lo split into f64)."""
    x = np.asarray(x).ravel()
    out = []
    for v in x:
        if np.iscomplexobj(x):
            out.append(mp.mpc(_mp_ld(v.real), _mp_ld(v.imag)))
        else:
            out.append(_mp_ld(v))
    return out


def _mp_ld(v):
    v = np.longdouble(v)
    if not np.isfinite(v):
        return mp.mpf(float(v))
    hi = np.float64(v)
    lo = np.float64(v - np.longdouble(hi))
    return mp.mpf(float(hi)) + mp.mpf(float(lo))


def _small(seed=23, m=8, n=4, b=3):
    return R.problem(seed, m, n, b)


def test_exact_G_makes_the_spec_the_nspace_iteration():
    """8 iterations from init, in mpmath: every output and every control decision of (b) equals (a)'s."""
    mp.mp.dps = R.DPS
    A, B, X0, Y0 = _small()
    par = dict(mu0=1.0, rho=2.0, tol_rel=0.2, tol_abs=1e-8, fixed_iters=False)
    ch = R.nspace_chain(A, X0, Y0, B, 8, ar=R.MP, **par)
    steps, fin = R.mspace_chain(ch.G, ch.K, A, B, X0, Y0, 8, ar=R.MP, **par)
    worst = mp.mpf(0)

    def close(x, y, what):
        nonlocal worst
        x, y = np.asarray(x).ravel(), np.asarray(y).ravel()
        num = max((abs(p - q) for p, q in zip(x, y)), default=mp.mpf(0))
        den = max((abs(q) for q in y), default=mp.mpf(0))
        if den == 0:
            assert num == 0, what
            return
        worst = max(worst, num / den)
        assert num <= mp.mpf(10) ** -25 * den, (what, mp.nstr(num / den, 5))

    seen = set()
    for k, o in enumerate(steps, 1):
        r, prev = ch.rec[k], ch.rec[k - 1]
        act = r["act"]
        assert np.array_equal(o["mask"]["run"], act), k
        if not act.any():
            continue
        v = o["val"]
        for name, ref in (("Yn", r["Y"]), ("M", r["M"]), ("En", r["e"]), ("AEn", r["AE"]), ("g", r["g"]), ("T", r["T"])):
            close(np.asarray(v[name])[act], np.asarray(ref)[act], (k, name))
        for name, ref in (("nep2", "nE2"), ("naz", "s"), ("nbeta", "an"), ("na", "alpha"), ("obj2", "obj2"),
                          ("nAX2", "nAX2"), ("nY2", "nY2"), ("nJM2", "nJM2"), ("dY2", "dY2"), ("jn2", "jn2"),
                          ("dZ2", "dZ2"), ("nX2", "nX2"), ("nZ2", "nZ2"), ("res_prim", "res_prim"),
                          ("res_comb", "res_comb"), ("t_prim", "t_prim"), ("t_comb", "t_comb")):
            close(np.asarray(v[name])[act], np.asarray(r[ref])[act], (k, name))
        # the iterate itself: X = c_v alpha X_init + A^H (c_v e + g)
        X = (v["cv"] * prev["alpha"])[:, None] * ch.Xinit + np.asarray(v["W"]) @ R.MP.conj(ch.A)
        close(X[act], r["Xcur"][act], (k, "X"))
        # decisions: improved, pending, and -- where the test was not left pending -- converged, stop, mu bump
        m_ = o["mask"]
        assert np.array_equal(m_["imp"], r["improved"]) and np.array_equal(m_["pendn"], r["pending"]), k
        np_ = act & ~r["pending"]
        assert np.array_equal(m_["conv"][np_], r["conv"][np_]) and np.array_equal(m_["bump"][np_], r["bump"][np_]), k
        # a pending test is finished by the next launch (or by fin): the dual part, the stop, the mu bump
        nxt = steps[k]["mask"] if k < len(steps) else fin["fin"]["mask"]
        nv = steps[k]["val"] if k < len(steps) else fin["fin"]["val"]
        p = r["pending"]
        if p.any():
            assert np.array_equal(nxt["pend_in"], p), k
            assert np.array_equal(nxt["dual_pass"][p], r["dual_pass"][p]) and np.array_equal(nxt["bump_in"][p], (r["bump"] & ~r["done"])[p]), k
            close(np.asarray(nv["res_dual"])[p], np.asarray(r["res_dual"])[p], (k, "res_dual"))
            close(np.asarray(nv["t_dual"])[p], np.asarray(r["t_dual"])[p], (k, "t_dual"))
        seen |= {n_ for n_ in ("imp", "pendn", "conv", "stop", "bump") if m_[n_].any()}
        seen |= {"not_" + n_ for n_ in ("imp", "bump") if (act & ~m_[n_]).any()}
        seen |= {n_ for n_ in ("dual_pass", "bump_in") if nxt[n_].any()}
    last = ch.rec[-1]
    close(fin["mu"], last["mu"], "mu")
    close(fin["X"], last["opt_X"], "opt_X")
    assert np.array_equal(fin["iters"], last["iters"]) and np.array_equal(fin["status"], last["status"])
    assert np.array_equal(fin["done"] != 0, last["done"])
    print(f"  (b) chained against (a) in mpmath: worst relative difference {mp.nstr(worst, 3)}; decisions met: "
          f"{sorted(seen)}")
    assert {"imp", "not_imp", "pendn", "bump", "not_bump", "conv", "stop", "bump_in"} <= seen, seen


def test_rounded_G_keeps_the_carried_state_within_its_bound():
    """G = fl64((I + K)^-1): the carried A E and ||E||^2 against the spec's own E = alpha X_init + A^H e obey
    d' = a_z d - R T with R = (I + K) G - I, so ||d'|| <= |a_z| ||d|| + ||R|| ||T||.  The bound is asserted against the
    spec's own E, where it is a theorem; against (a) the trajectories themselves differ by the perturbation of G, which
    that recursion does not bound, so (a)'s deviation is printed and held to 1e-15 relative (measured 9e-17)."""
    ld = R.LD
    for (m, n, b) in ((40, 16, 5), (121, 64, 3)):
        A, B, X0, Y0 = R.problem(31, m, n, b)
        par = dict(mu0=4.0, rho=1.05, tol_rel=1e-4, tol_abs=1e-8, fixed_iters=True)
        ch = R.nspace_chain(A, X0, Y0, B, 8, ar=ld, **par)
        G64 = ld.f64(ch.G)
        Rm = (np.eye(m) + ch.K) @ ld.c(G64) - np.eye(m)
        nR = float(np.linalg.norm(Rm.astype(np.complex128), 2)) * 1.0001 + 1e-19 * m
        steps, fin = R.mspace_chain(G64, ld.f64(ch.K), A, B, X0, Y0, 8, ar=ld, **par)
        A_ = ld.c(A)
        bound, nbound = np.zeros(b, np.longdouble), np.zeros(b, np.longdouble)
        az = np.abs(R.mspace_init(X0, X0 @ A.T, ld)["naz"])            # |a_z| of the step: E' = a_z E + A^H g
        worst = worst_n = dev_a = 0.0
        norm = lambda x: np.sqrt(np.sum(np.abs(x) ** 2, axis=1))
        for k, o in enumerate(steps, 1):
            v, S = o["val"], o["state"]
            nT, ng = norm(v["T"]), norm(v["g"])
            nbound = az * az * nbound + 2 * az * bound * ng + ng * nR * nT
            bound = az * bound + nR * nT
            E = np.asarray(S["na"])[:, None] * ld.c(X0) + np.asarray(v["En"]) @ np.conj(A_)
            d = norm(np.asarray(v["AEn"]) - E @ A_.T)
            dn = np.abs(np.asarray(v["nep2"]) - np.sum(np.abs(E) ** 2, axis=1))
            slack = 64 * 2.0 ** -64 * m * (norm(E @ A_.T) + 1)           # longdouble rounding of this check itself
            assert np.all(d <= bound + slack), (k, d, bound)
            assert np.all(dn <= nbound + slack * (norm(E) + 1)), (k, dn, nbound)
            worst, worst_n = max(worst, float(np.max(d / (bound + slack)))), max(worst_n, float(np.max(dn / (nbound + slack))))
            az = np.abs(np.asarray(S["naz"]))
            r = ch.rec[k]
            dev_a = max(dev_a, float(np.max(norm(np.asarray(v["AEn"]) - r["AE"]) / norm(r["AE"]))),
                        float(np.max(np.abs(np.asarray(v["nep2"]) - r["nE2"]) / r["nE2"])))
        print(f"  m {m}: ||(I+K)G - I|| = {nR:.3g}; carried A E / ||E||^2 use {worst:.3g} / {worst_n:.3g} of the "
              f"propagated bound; relative deviation from the n-space truth after 8 iterations {dev_a:.3g}")
        assert dev_a < 1e-15


EXPECT = {   # what each input was built for: mask name -> "all" | "some" | "none" over the run (or live) realisations
    "m1-n4-b1-k0": dict(imp="all"),
    "m16-n16-b15-k1": dict(imp="none", bump="none"),
    "m31-n16-b16-k5": dict(bump="some"),
    "m33-n16-b17-k30": dict(bump="some"),
    "m40-n16-b33-k1-done": dict(imp="none"),
    "m40-n4-b17-k5-alldone": dict(),
    "m121-n16-b17-k0": dict(imp="all"),
    "m121-n64-b16-k30": dict(bump="some"),
    "m225-n64-b15-k5": dict(bump="some"),
    "m256-n64-b16-k1": dict(bump="none"),
    "m256-n64-b17-k5-mu1e-3": dict(shrunk0="all"),
    "m40-n16-b16-fixpoint": dict(conv="some", stop="none", bump="some"),
    "m40-n16-b16-fixpoint-stop": dict(conv="some", stop="some"),
    "m256-n64-b16-fixpoint": dict(conv="all", stop="none"),
    "m33-n16-b17-pending": dict(pend_in="some", dual_pass="none", bump_in="none", pendn="some"),
    "m33-n16-b17-pending-bump": dict(pend_in="some", dual_pass="none", bump_in="some"),
    "m33-n16-b17-pending-pass": dict(pend_in="some", dual_pass="some", stop_in="some"),
    "m33-n16-b17-pending-pass-fixed": dict(pend_in="some", dual_pass="some", stop_in="none"),
    "m40-n16-b17-k0-nanB": dict(cur="some", imp="some"),
    "m121-n64-b16-k30-imp": dict(imp="all"),
    "m33-n16-b17-k5-imp-nanB": dict(imp="some", cur="some"),
    "m31-n16-b16-k5-nX2": dict(conv="some", pendn="some"),
}


def test_every_input_shows_its_case_away_from_ties():
    assert set(EXPECT) == set(R.CASES)
    covered = set()
    for name in R.CASES:
        inp = R.case(name)
        o = R.mspace_step(inp)
        msk = o["mask"]
        base = msk["run"]
        for k, want in EXPECT[name].items():
            got = msk[k]
            dom = msk["live"] if k in ("pend_in", "dual_pass", "stop_in", "bump_in") else base
            if want == "all":
                assert got[dom].all() and dom.any(), (name, k)
            elif want == "some":
                assert got.any(), (name, k)
            else:
                assert not got.any(), (name, k)
        for k in ("imp", "pendn", "conv", "stop", "bump", "cur", "shrunk0", "dual_pass", "stop_in", "bump_in"):
            if msk[k].any():
                covered.add(k)
            if (base & ~msk[k]).any():
                covered.add("not_" + k)
        if (msk["pend_in"] & ~msk["dual_pass"]).any():
            covered.add("dual_fail")
        # the done rows and the ragged block ends are what the name says
        done = inp["flags"][:, 1] != 0
        assert set(np.flatnonzero(done)) >= set(R.DONE_ROWS.get(name, ())), name
        low = {}
        for k, mg in o["margin"].items():
            fin = mg[np.isfinite(mg)]
            if fin.size:
                low[k] = float(fin.min())
        nanrow = np.isnan(R.LD.f64(o["val"]["obj2"]).astype(np.float64)) & base
        assert nanrow.sum() == (1 if name in R.NAN_B else 0), name
        print(f"  {name}: live {int(msk['live'].sum())} run {int(base.sum())}; smallest decision margins "
              + ", ".join(f"{k} {v:.2g}" for k, v in sorted(low.items())))
        assert all(v >= 1e-6 for v in low.values()), (name, low)
        # every decision is also outside the tolerance of the quantity it compares
        rc, src = R.LD.f64(o["val"]["res_comb"]).astype(np.float64), R.LD.f64(o["scale"]["res_comb"]).astype(np.float64)
        with np.errstate(all="ignore"):
            relerr = R.TOL_MULT * R.U * src / rc
        ok = base & ~nanrow
        assert np.all(relerr[ok] < o["margin"]["combined"][ok]), (name, relerr[ok].max())
        upd = ok & np.isfinite(o["margin"]["bump"])
        assert np.all(relerr[upd] < o["margin"]["bump"][upd]), name
    want = {"imp", "not_imp", "pendn", "conv", "stop", "not_stop", "bump", "not_bump", "cur", "shrunk0", "not_shrunk0",
            "dual_pass", "dual_fail", "stop_in", "bump_in"}
    print(f"  branches covered by the suite's inputs: {sorted(covered)}")
    assert want <= covered, want - covered


def test_oracle_ratio():
    """The f64 transcription of (b) against (b): the largest err / (u S) over the suite's inputs is ORACLE_RATIO."""
    worst, where = 0.0, None
    for name in R.CASES:
        inp = R.case(name)
        ref, f64 = R.mspace_step(inp), R.mspace_step(inp, R.F64)
        _same_decisions(ref, f64)
        for k, v in _ratios(ref, f64).items():
            if v > worst:
                worst, where = v, (name, k)
    print(f"  f64 transcription: worst err / (u S) = {worst:.4g} at {where}; ORACLE_RATIO = {R.ORACLE_RATIO}, "
          f"TOL_MULT = {R.TOL_MULT}")
    assert 0.75 * R.ORACLE_RATIO <= worst <= R.ORACLE_RATIO
    assert R.TOL_MULT == 8.0 * R.ORACLE_RATIO


MODEL_INPUTS = {   # the inputs of the GPU suite on which each wrong step must show
    "G_transposed": ("m16-n16-b15-k1", "m256-n64-b16-k1"),
    "cv_times_mu": ("m31-n16-b16-k5",),
    "stale_mu": ("m33-n16-b17-pending-bump",),
    "AE_without_Kg": ("m16-n16-b15-k1",),
    "hp1_nE2": ("m31-n16-b16-k5",),
    "hp1_nX2": ("m31-n16-b16-k5-nX2",),
    "hp1_jn2": ("m31-n16-b16-k5", "m40-n16-b16-fixpoint"),
    "hp1_dZ2": ("m31-n16-b16-k5", "m40-n16-b16-fixpoint"),
    "dY2_wrong_buffer": ("m31-n16-b16-k5",),
    "optW_az": ("m121-n64-b16-k30-imp", "m33-n16-b17-k5-imp-nanB"),
    "pad_in_sums": ("m31-n16-b16-k5", "m225-n64-b15-k5"),
    "swap_jl4": ("m33-n16-b17-k30",),
}


def test_wrong_step_models_fail_the_comparisons_of_the_gpu_suite():
    """Each model's result, laid out as the device leaves it, goes through nms_ref.compare_step -- the comparisons, row
    masks and tolerances of tests/test_gpu_nms.py::check_step, nothing else: an output the device run compares lands at
    least 10 x outside its tolerance, or an exact comparison (a decision, mu) breaks.  The right step passes them."""
    assert set(MODEL_INPUTS) == set(R.MODELS)
    for model, names in MODEL_INPUTS.items():
        for name in names:
            assert name in R.CASES
            inp = R.case(name)
            ratios, broken, _ = R.compare_step(R.model_result(inp), inp)
            assert not broken and max(v for _, v in ratios) <= 1.0 / 8.0, (name, broken, ratios)
            ratios, broken, _ = R.compare_step(R.model_result(inp, model), inp)
            k, sep = max(ratios, key=lambda kv: kv[1])
            print(f"  {model} on {name}: {k} is {sep:.3g} x the tolerance; exact comparisons broken: {broken}")
            if model == "hp1_nX2":      # ||X||^2 reaches only the thresholds: it is caught by the decision it flips
                assert {"flag done", "flag status", "done_count"} <= set(broken), (model, name, broken)
                right, wrong = R.mspace_step(inp), R.mspace_step(inp, model=model)
                for o in (right, wrong):   # ... with both sides away from a tie
                    assert float(np.nanmin(o["margin"]["combined"])) >= 1e-6
                j = R.NX2_ROW
                assert right["mask"]["conv"][j] != wrong["mask"]["conv"][j]
            else:
                assert sep >= 10.0, (model, name, ratios)


def test_recorded_iterate_deviation():
    """V + A^H Wsel of an iterate recorded past init against the n-space truth's X: the f64 transcription's own
    deviation is REC_DEV; the kernel gets CHAIN_MULT x (tests/test_gpu_nms.py)."""
    worst = 0.0
    for name in R.RECORDED:
        inp = R.case(name)
        got = R.model_result(inp)
        A, X0, truth = R.recorded_truth(name)
        imp = R.mspace_step(inp)["mask"]["imp"]
        co = np.where(imp, got.state[:, R.SI["nopt_a"]], got.state[:, R.SI["ncur_a"]])[:, None]
        Wsel = np.where(imp[:, None], got.vec["optW"], got.vec["curW"])
        dev = R.recorded_deviation(X0 * co, Wsel, A, truth)
        bad = R.model_result(inp, "optW_az")
        dev_bad = R.recorded_deviation(X0 * co, np.where(imp[:, None], bad.vec["optW"], bad.vec["curW"]), A, truth)
        print(f"  {name}: f64 transcription {dev:.3g}; with optW = a_z e + g {dev_bad:.3g}")
        assert dev_bad >= 10 * R.CHAIN_MULT * R.REC_DEV
        worst = max(worst, dev)
    print(f"  REC_DEV = {R.REC_DEV}, measured {worst:.3g}")
    assert 0.25 * R.REC_DEV <= worst <= R.REC_DEV


def test_chain_deviation():
    """5 steps from init, fin and out: the f64 transcription's own deviation from the n-space truth on the chains of the
    GPU suite (assertion 6) is CHAIN_DEV; the kernel gets CHAIN_MULT x."""
    worst = dict(y=0.0, x=0.0, scal=0.0)
    for name, (seed, m, n, b) in R.CHAINS.items():
        ch = R.chain(seed, m, n, b, R.CHAIN_STEPS)
        A, B, X0, Y0 = R.problem(seed, m, n, b)
        G, K = R.LD.f64(ch.G), R.LD.f64(ch.K)
        steps, fin = R.mspace_chain(G, K, A, B, X0, Y0, R.CHAIN_STEPS, ar=R.F64, **R.CHAIN_PAR)
        last = ch.rec[R.CHAIN_STEPS]
        assert np.array_equal(fin["iters"], last["iters"]) and np.array_equal(fin["status"], last["status"])
        assert np.array_equal(np.asarray(fin["mu"], np.float64), R.LD.f64(last["mu"]))
        dev = R.chain_deviation(steps, fin, ch)
        low = min(float(np.nanmin(mg[np.isfinite(mg)])) for o in R.mspace_chain(G, K, A, B, X0, Y0, R.CHAIN_STEPS, ar=R.LD,
                  **R.CHAIN_PAR)[0] for mg in o["margin"].values() if np.isfinite(mg).any())
        print(f"  {name}: smallest decision margin over the chain's steps {low:.2g}")
        assert low >= 1e-6
        print(f"  {name}: f64 chain against the n-space truth: " + ", ".join(f"{k} {v:.3g}" for k, v in dev.items()))
        for k in worst:
            worst[k] = max(worst[k], dev[k])
    print(f"  CHAIN_DEV = {R.CHAIN_DEV}, measured {worst}")
    for k in worst:
        assert 0.25 * R.CHAIN_DEV[k] <= worst[k] <= R.CHAIN_DEV[k], (k, worst[k])


def test_cancellation_case_is_reported():
    """The largest kappa of res_comb and nep2' on the near-fixed-point inputs, the relative error the tolerance allows
    there, and the margin of the stop test on the default chain (tol_rel = 1e-4) at its stopping iterations."""
    for name in ("m40-n16-b16-fixpoint", "m256-n64-b16-fixpoint"):
        o = R.mspace_step(R.case(name))
        f = lambda k: float(np.max(np.asarray(o["scale"][k] / np.abs(o["val"][k]), np.float64)))
        print(f"  {name}: kappa(res_comb) {f('res_comb'):.3g}, kappa(jn2) {f('jn2'):.3g}, kappa(dZ2) {f('dZ2'):.3g}, "
              f"kappa(nep2') {f('nep2'):.3g}; allowed relative error of res_comb {R.TOL_MULT * R.U * f('res_comb'):.3g}")
    seed, m, n, b = 13, 33, 16, 17
    ch = R.chain(seed, m, n, b, 80)
    worst_k, low = 0.0, np.inf
    for k in range(1, 80):
        o = R.mspace_step(ch.mspace(k))
        run = o["mask"]["run"]
        if not run.any():
            break
        kap = np.asarray(o["scale"]["res_comb"] / o["val"]["res_comb"], np.float64)
        near = run & (o["margin"]["combined"] < 0.5)
        if near.any():
            worst_k = max(worst_k, float(kap[near].max()))
            low = min(low, float(o["margin"]["combined"][near].min()))
    print(f"  default chain (m {m}, tol_rel 1e-4): where res_comb is within a factor 2 of its threshold, kappa(res_comb) "
          f"<= {worst_k:.3g} (relative error bound {R.TOL_MULT * R.U * worst_k:.3g}), closest margin {low:.3g}")
    assert R.TOL_MULT * R.U * worst_k < low      # the error the tolerance allows cannot reach the closest decision
