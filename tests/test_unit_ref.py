"""CPU tests of tests/unit_ref.py, the references of tests/test_gpu_unit.py: the tolerance unit (the f64 transcription
against the longdouble specification), the decision margins of every input the GPU suite uses, the specification
against the n-space truth, and the wrong-step models, each of which must exceed its tolerance on some input through
the compare function the GPU test uses.  No GPU, no project code."""
import functools

import numpy as np
import pytest

import unit_ref as R

RUNS = [("m256-n64-b35", v) for v in R.RUN_VARIANTS] + [("m256-n64-b16", "end"), ("m256-n64-b16", "midstop")]


@functools.lru_cache(maxsize=None)
def _both(name):
    inp = R.case(name)
    return inp, R.step(inp), R.step(inp, R.F64)


def test_the_tables_match_the_python_mirror():
    from ace_amd import ustep
    assert R.STATE == ustep.STATE and R.FLAGS == ustep.FLAGS and R.VEC_M == ustep.VEC_M and R.VEC_N == ustep.VEC_N


def test_oracle_ratio():
    """The tolerance unit: the worst err / (u S) of the f64 transcription of (b) against (b) in longdouble over the
    step inputs, floored at 1, is ORACLE_RATIO (rounded up, by less than a quarter)."""
    worst, where = {}, {}
    for name in R.CASES:
        inp, ref, f64 = _both(name)
        ratios, broken, _ = R.compare_step(R.FakeResult(f64, R.F64), inp, ref, mult=1.0)
        assert not broken, (name, broken)
        for k, v in ratios:
            k = "Y'" if k in ("Y0", "Y1") else "S'" if k in ("S0", "S1") else "Z'" if k in ("Zb1", "Zb2") else k
            if v > worst.get(k, 0.0):
                worst[k], where[k] = v, name
    for k in sorted(worst):
        print(f"  f64 transcription, err / (u S) of {k}: {worst[k]:.3g} ({where[k]})")
    unit = max(1.0, max(worst.values()))
    print(f"  unit {unit:.4g}, ORACLE_RATIO {R.ORACLE_RATIO}, TOL_MULT {R.TOL_MULT}")
    assert unit <= R.ORACLE_RATIO <= 1.25 * unit and R.TOL_MULT == 8.0 * R.ORACLE_RATIO


def _margins_hold(ref, f64, label):
    """Every decision the launch takes is the same in f64 and longdouble and lies at least 64 x their distance from
    a tie."""
    for k, v in ref["mask"].items():
        assert np.array_equal(v, f64["mask"][k]), (label, k)
    for k, mg in ref["margin"].items():
        m64 = f64["margin"][k]
        ev = np.isfinite(mg)
        assert np.array_equal(np.isnan(mg), np.isnan(m64)), (label, k)
        if ev.any():
            dist = np.abs(mg[ev] - m64[ev])
            assert np.all(mg[ev] >= 64.0 * dist) and np.all(mg[ev] > 1e-9), (label, k, float(mg[ev].min()), float(dist.max()))


@pytest.mark.parametrize("name", list(R.CASES))
def test_decision_margins_of_the_step_inputs(name):
    inp, ref, f64 = _both(name)
    _margins_hold(ref, f64, name)
    assert np.array_equal(R.pack_flags(ref["flags"]), R.pack_flags(f64["flags"])), name
    assert (ref["done_count"], ref["mspcount"]) == (f64["done_count"], f64["mspcount"])


@pytest.mark.parametrize("shape,variant", RUNS)
def test_decision_margins_of_the_run_inputs(shape, variant):
    """Every iteration of the reference's run, stepped in longdouble and in f64 from the same f64 state."""
    inp = R.run_case(shape, variant)
    seen = []

    def stepper(cur):
        a, b = R.step(cur), R.step(cur, R.F64)
        _margins_hold(a, b, (shape, variant, cur["it"]))
        seen.append(cur["it"])
        return a

    r = R.run(inp, stepper=stepper)
    plain = R.run(inp)
    assert (r["resume"], r["steps"], r["vecw"]) == (plain["resume"], plain["steps"], plain["vecw"])
    f64 = R.run(inp, R.F64)
    assert (r["resume"], r["steps"], r["vecw"], r["done_count"]) == (f64["resume"], f64["steps"], f64["vecw"], f64["done_count"])
    assert np.array_equal(r["flags"], f64["flags"])
    if variant not in ("allstop",):
        assert seen and seen[0] == inp["it"]


def test_the_inputs_reach_every_branch():
    """What the GPU suite's inputs exercise, counted on the reference: every role runs, and every rare branch of the
    issue is taken by at least two realisations somewhere."""
    tot = {}
    for name in R.CASES:
        _, ref, _ = _both(name)
        for k, v in ref["mask"].items():
            tot[k] = tot.get(k, 0) + int(v.sum())
    for k in ("pend_in", "stop_in", "bump_in", "dual_pass", "la_rows", "avok", "cand", "ent", "take", "ctl", "bound_fail",
              "conv", "stop", "bump", "imp", "imp_ctl", "ah", "el", "ah_save"):
        assert tot.get(k, 0) >= 2, (k, tot)
    inp, ref, _ = _both("entry-m17")
    en = np.array([r == "enter" for r in inp["roles"]])
    assert np.array_equal(ref["mask"]["take"], en) and ref["mask"]["cand"].all()      # room, and no room
    inp, ref, _ = _both("defer-m17")
    assert ref["copied"]["optY"].sum() >= 2 and ref["copied"]["optS"].sum() >= 2
    z = R.step(R.zero_guard_case())
    assert z["mask"]["zero_guard"].all()
    a = R.step(R.ahead_case())
    assert not a["mask"]["act"][:16].any() and a["mask"]["act"][16:].all()
    p = R.run(R.run_case("m256-n64-b35", "pending"))
    assert p["steps"][3] == 3 and p["resume"] == p["it_last"] + 1
    fb = R.run(R.run_case("m256-n64-b35", "failbound"))
    assert fb["steps"][2] == 3 and fb["resume"] == fb["it_last"]
    ms = R.run(R.run_case("m256-n64-b35", "midstop"))
    assert ms["done_count"] == 2 and ms["it_last"] == 13 and ms["resume"] == 14
    stopped = ms["flags"][:, R.FLAGS.index("done")] != 0                # mid-run, at the other parity from the run's end
    assert stopped.sum() == 2 and np.all(ms["flags"][stopped, R.FLAGS.index("iters")] == 10)
    nr = R.run(R.run_case("m256-n64-b35", "notready"))
    assert nr["steps"][1] == 1 and nr["resume"] == 9 and not nr["ran"][32:].any()
    ah = R.run(R.run_case("m256-n64-b35", "ahead"))
    assert ah["resume"] == 12 and not ah["ran"][:16].any()


@pytest.mark.parametrize("name", ["gyf-m17-n33-b17", "gyfm-m17-n33-b17", "gyfm-m121-n256-b35", "entry-m17", "defer-m17",
                                  "mixed-block-m17", "gyfm-m243-n64-b16"])
def test_the_specification_agrees_with_the_nspace_truth(name):
    """(b) in longdouble against (a): within the bound the GPU test uses, with room to spare (the specification's own
    distance from the truth is the allowance's, not the tolerance's)."""
    inp, ref, _ = _both(name)
    ratios, _, tr = R.compare_truth(R.FakeResult(ref), inp)
    for k, v in ratios:
        print(f"  {name}: {k} {v:.3g}")
    assert all(v <= 0.5 for _, v in ratios), ratios
    # and the certificate's claim on the realisations whose control ran: ArgMinZ leaves X as it is
    O = R._oracle()
    m, n = inp["A"].shape
    tx = max(d for d in range(1, int(np.sqrt(n)) + 1) if n % d == 0)
    ctl = ref["mask"].get("ctl", np.zeros(len(inp["roles"]), bool))
    for j in np.nonzero(ctl)[0][:4]:
        X = R.F64.c(R.LD.f64(tr["X"][j]))[:, None]
        Zs = O.argmin_z_lowrank(X.copy(), np.zeros_like(X), 1.0, tx, n // tx, m, n, False)
        assert np.array_equal(Zs, X), (name, j)


MODEL_INPUTS = {
    "stale_mu": ["pend-stop-m17", "gykL-m121-n256-b35"],
    "S_not_reset": ["entry-m17", "gyfm-m121-n256-b35"],
    "optY_from_Yo": ["gykT-m17-n33-b17", "gyf-m17-n33-b17"],
    "pad_in_sums": ["gyf-m17-n33-b17", "gyk-m243-n64-b16"],
    "fs0_no_2": ["entry-m17", "defer-m121"],
    "fs3_from_gg": ["entry-m17", "defer-m121"],
    "kfcum_no_room": ["entry-m17", "entry-m121"],
}


@pytest.mark.parametrize("model", list(MODEL_INPUTS))
def test_wrong_step_models_exceed_the_tolerance(model):
    """Each mutated reference, through the GPU test's compare function: outside the tolerance (or an exact comparison
    broken) on every input listed for it."""
    for name in MODEL_INPUTS[model]:
        inp, ref, _ = _both(name)
        wrong = R.step(inp, model=model)
        ratios, broken, _ = R.compare_step(R.FakeResult(wrong), inp, ref)
        worst = max([v for _, v in ratios] + [0.0])
        print(f"  {model} on {name}: worst err/tol {worst:.3g}, exact comparisons broken {broken}")
        assert worst > 1.0 or broken, (model, name)


def test_the_zero_guard_model_is_caught():
    inp = R.zero_guard_case()
    ref = R.step(inp)
    ratios, broken, _ = R.compare_step(R.FakeResult(R.step(inp, model="no_zero_guard")), inp, ref)
    assert max(v for _, v in ratios) > 1.0
    ratios, broken, _ = R.compare_step(R.FakeResult(R.step(inp, R.F64), R.F64), inp, ref)
    assert not broken and max(v for _, v in ratios) <= 1.0


@pytest.mark.parametrize("model", ["wb_parity", "resume_plus1", "fs0_no_2"])
def test_wrong_run_models_are_caught(model):
    """The run's write-back parity, its resume point after a failed bound and a wrong shared helper, through
    compare_run_chain, the comparison the GPU test makes between a run and the chain of gyf launches."""
    inp = R.run_case("m256-n64-b35", "failbound")
    ref = R.run(inp)
    assert not R.compare_run_chain(R.FakeResult(ref), inp, ref)
    wrong = R.run(inp, model=model)
    broken = R.compare_run_chain(R.FakeResult(wrong), inp, ref)
    print(f"  {model}: differs in {broken}")
    assert broken
    if model == "resume_plus1":
        assert "resume" in broken
    if model == "wb_parity":
        assert {"Y0", "Y1", "S0", "S1"} <= set(broken) and "resume" not in broken
