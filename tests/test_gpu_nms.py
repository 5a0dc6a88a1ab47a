"""The A2nuclear m-space iteration kernel (nms_kernel, csrc/ace_nucmsp.hip) one launch at a time, against the references
of tests/nms_ref.py: (b) the m-space specification in longdouble on exactly the kernel's f64 inputs, with a condition
number per output, and (a) the n-space truth, InferADMM of inferLowRank_Nuclear.m at r = 1.

Everything goes through the test entry ace_nms_host (ace_amd.nms), which fills the kernel's argument blocks and one
control block per realisation as the solve does and calls the solve's launchers: launch_nms_init, launch_gyk_gfrag of
the dense G and K followed by launch_nms (an iteration, or only the pending convergence tests), launch_nms_out.

Assertions (numbered as in DESIGN section 6): 1 a step against (b), every vector elementwise and every sum, state
field and flag; 2 each control branch; 3 a convergence test pending on entry, and fin; 4 known answers that need no
reference; 5 init and out (also of an iterate recorded past init, against (a)'s X); 6 a chain of 5 steps from init, with fin and out, against (a); 7 isolation and untouched
memory.  Tolerances are TOL_MULT u kappa |value| (nms_ref: TOL_MULT is 8 x the f64 transcription's own worst ratio);
every comparison states err / tol (printed; the worst per output is printed when the module finishes and recorded in
DESIGN).  The inputs, their branches and their decision margins are shown on the reference alone by
tests/test_nms_ref.py.

Measured on the MI355X: worst err / tol 0.24 (e' and optW at m = 121), 0.17 (A E_new), 0.087 (Y'), below 0.03 for
every sum and state field; the chains use 0.07 - 0.20 of their bound, out of a recorded iterate 0.17; at the largest kappa(res_comb) = 2.8e9 (the
near-fixed-point state at m = 256) the relative error of res_comb is 4.4e-11.
"""
import functools

import numpy as np
import pytest

import nms_ref as R

pytestmark = pytest.mark.gpu

WORST = {}      # output -> (worst err / tol seen, where)
CANCEL = {}     # the largest kappa(res_comb) seen, with the relative error of res_comb measured there
SI = {k: i for i, k in enumerate(R.STATE)}
FI = {k: i for i, k in enumerate(R.FLAGS)}


class _Entry:
    """ace_amd.nms with one rule added: a HIP error ends the session (nothing more is launched on a device that has
    reported a fault)."""

    def __init__(self):
        from ace_amd import nms
        self._n = nms
        self.SENTINEL = nms.SENTINEL

    def nms_host(self, *a, **kw):
        from ace_amd import AceError
        try:
            return self._n.nms_host(*a, **kw)
        except AceError as e:
            if e.code == -3:
                pytest.exit(f"HIP error in ace_nms_host: {e}", returncode=3)
            raise


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module's tests: the worst err / tol per output over the comparisons that ran (pytest -s shows them).
    Every figure was asserted where it was measured; nothing is asserted here."""
    yield
    for k in sorted(WORST):
        print(f"  worst err/tol {k}: {WORST[k][0]:.3g} ({WORST[k][1]})")
    if CANCEL:
        print(f"  largest kappa(res_comb) {CANCEL['kappa']:.3g} at {CANCEL['where']}: relative error of res_comb "
              f"{CANCEL['rel']:.3g}, kappa(nep2') {CANCEL['kappa_nep2']:.3g}")


def _bits(a):
    return np.ascontiguousarray(a).view(np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.all(_bits(a) == _bits(b)))


def _is_sentinel(x, s):
    return bool(np.all(np.ascontiguousarray(x).view(np.float64) == s))


def _kw(inp, **over):
    b, m = inp["Yo"].shape
    kw = dict(batch=b, n=inp["n"], m=m, it=inp["it"], fixed_iters=inp["fixed_iters"], tol_rel=inp["tol_rel"],
              tol_abs=inp["tol_abs"], rho=inp["rho"], done_count=inp["done_count"])
    for k in ("G", "K", "B", "Yo", "Yn", "M", "Eo", "AEo", "optW", "optY", "curW", "state", "flags"):
        kw[k] = inp[k]
    kw.update(over)
    return kw


def _within(got, ref, scale, rows, out, label):
    """|got - ref| <= TOL_MULT u scale on the given rows; records err / tol under `out`."""
    got = np.asarray(got)[rows].astype(np.clongdouble)
    ref = np.asarray(ref)[rows].astype(np.clongdouble)
    tol = R.tolerance(np.asarray(scale)[rows])
    if not got.size:
        return
    assert np.all(np.isfinite(got.view(np.longdouble))), f"{label}: {out} is not finite"
    err = np.abs(got - ref)
    with np.errstate(all="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    print(f"  {label}: {out} err/tol {worst:.3g}")
    if worst > WORST.get(out, (0.0, ""))[0]:
        WORST[out] = (worst, label)
    assert worst <= 1.0, f"{label}: {out} is {worst:.3g} x its tolerance"


def _untouched(res, guard_names, label, sentinel):
    for k in guard_names:
        assert _is_sentinel(res.guards[k], sentinel), f"{label}: the guard after {k} was written"
    assert res.guard_ok, f"{label}: a control-block field outside the iteration's own was written"


def check_step(res, inp, label, sentinel, fin=False):
    """Assertions 1, 2, 3 and 7 on one launch: everything the launch wrote against (b), everything else untouched.
    The comparisons themselves are nms_ref.compare_step, the function through which tests/test_nms_ref.py measures
    the wrong-step models."""
    _untouched(res, res.guards.keys(), label, sentinel)
    ratios, broken, ref = R.compare_step(res, inp, fin=fin)
    msk = ref["mask"]
    for k in ("En", "AEn"):
        rows_ = np.ones(len(msk["run"]), bool) if fin else ~msk["run"]
        assert _is_sentinel(res.vec[k][rows_], sentinel), f"{label}: {k} of a realisation that takes no step was written"
    for out, worst in ratios:
        print(f"  {label}: {out} err/tol {worst:.3g}")
        if worst > WORST.get(out, (0.0, ""))[0]:
            WORST[out] = (worst, label)
    assert not broken, f"{label}: exact comparisons that do not hold: {broken}"
    bad = [(o, f"{w:.3g}") for o, w in ratios if not w <= 1.0]
    assert not bad, f"{label}: outside the tolerance (output, err/tol): {bad}"
    if not fin:
        val, sc = ref["val"], ref["scale"]
        nanrow = msk["run"] & np.isnan(R.LD.f64(val["obj2"]).astype(np.float64))
        rws = msk["run"] & ~msk["pendn"] & ~msk["stop"] & ~nanrow
        if rws.any():                              # the cancellation of the quadratic forms, as measured
            rc = np.asarray(val["res_comb"], np.longdouble)[rws]
            rel = float(np.max(np.abs(res.last_res[rws].astype(np.longdouble) - rc) / rc))
            kap = float(np.max(np.asarray(sc["res_comb"], np.longdouble)[rws] / rc))
            kne = float(np.max(np.asarray(sc["nep2"], np.longdouble)[rws] / np.asarray(val["nep2"], np.longdouble)[rws]))
            print(f"  {label}: kappa(res_comb) <= {kap:.3g}, kappa(nep2') <= {kne:.3g}, relative error of res_comb {rel:.3g}")
            if kap > CANCEL.get("kappa", 0.0):
                CANCEL.update(kappa=kap, kappa_nep2=kne, rel=rel, where=label)
    return ref


@functools.lru_cache(maxsize=None)
def _launch(name):
    e = _Entry()
    inp = R.case(name)
    return e.nms_host("step", **_kw(inp)), inp, e.SENTINEL


# ------------------------------------------------------------------ 1, 2: a step against the specification
@pytest.mark.parametrize("name", list(R.CASES))
def test_step_matches_the_specification(name):
    res, inp, sent = _launch(name)
    ref = check_step(res, inp, name, sent)
    msk = ref["mask"]
    print(f"  {name}: run {int(msk['run'].sum())}, improved {int(msk['imp'].sum())}, pending {int(msk['pendn'].sum())}, "
          f"converged {int(msk['conv'].sum())}, stopped {int(msk['stop'].sum())}, mu bumped {int(msk['bump'].sum())}")


def test_each_control_branch_on_the_device():
    """2: what the device's own flags and buffers say on the inputs built for each branch."""
    conv = R.ST_CONVERGED
    res, inp, sent = _launch("m121-n16-b17-k0")                        # improved: every realisation records its iterate
    assert not _is_sentinel(res.vec["optW"], sent) and np.all(res.opt_obj < np.inf) and np.all(res.iters == 1)
    cv_al = inp["state"][:, SI["naz"]] * inp["state"][:, SI["na"]]     # a_n = 0 after init: c_v = a_z
    assert _same(res.nopt_a, cv_al)
    res, inp, sent = _launch("m16-n16-b15-k1")                         # not improved, mu not bumped
    assert _same(res.vec["optW"], inp["optW"]) and _same(res.mu, inp["state"][:, SI["mu"]])
    res, inp, sent = _launch("m40-n16-b17-k0-nanB")                    # NaN objective with opt_obj = +inf
    j = R.NAN_B["m40-n16-b17-k0-nanB"][0]
    assert np.isnan(res.obj2[j]) and res.opt_obj[j] == np.inf and res.dpend[j] == 0 and res.done[j] == 0
    assert np.all(np.isfinite(res.vec["curW"][j].view(np.float64))) and _same(res.vec["optW"][j], inp["optW"][j])
    assert res.ncur_a[j] == inp["state"][j, SI["naz"]] * inp["state"][j, SI["na"]] and np.isnan(res.last_res[j])
    others = np.arange(17) != j
    assert _same(res.vec["curW"][others], inp["curW"][others])
    res, inp, sent = _launch("m40-n16-b16-fixpoint-stop")              # converged and stopping
    stopped = res.done != 0
    assert stopped.sum() == res.done_count - inp["done_count"] > 0 and np.all(res.status[stopped] & conv)
    assert _same(res.mu[stopped], inp["state"][stopped, SI["mu"]]), "a stopping realisation keeps its mu"
    assert _same(res.last_res[stopped], inp["state"][stopped, SI["last_res"]])
    res2, inp2, _ = _launch("m40-n16-b16-fixpoint")                    # the same under fixed_iters
    assert np.all(res2.done == 0) and res2.done_count == inp2["done_count"]
    assert np.array_equal((res2.status & conv) != 0, stopped) and not _same(res2.mu, inp2["state"][:, SI["mu"]])
    for k in ("Yn", "M", "En", "AEn"):                                 # and it computes what the stopping launch did
        assert _same(res2.vec[k], res.vec[k]), k
    res, inp, sent = _launch("m33-n16-b17-pending")                    # pending set
    pn = (res.dpend != 0) & (inp["flags"][:, FI["dpend"]] == 0)
    assert pn.any() and _same(res.mu[pn], inp["state"][pn, SI["mu"]]) and np.all(res.pd_rc[pn] > 0)
    res, inp, sent = _launch("m31-n16-b16-k5")                         # mu bumped by rho, and not
    up = res.mu != inp["state"][:, SI["mu"]]
    assert up.any() and (~up).any() and _same(res.mu[up], inp["state"][up, SI["mu"]] * np.float64(inp["rho"]))


# ------------------------------------------------------------------ 3: a pending test on entry, and fin
def test_pending_test_on_entry():
    conv = R.ST_CONVERGED
    res, inp, sent = _launch("m33-n16-b17-pending-pass")               # the dual part passes: the realisation stops
    p = inp["flags"][:, FI["dpend"]] != 0
    assert p.sum() >= 2 and np.all(res.done[p] == 1) and np.all(res.status[p] & conv) and np.all(res.dpend[p] == 0)
    assert res.done_count - inp["done_count"] >= p.sum()
    assert _is_sentinel(res.vec["En"][p], sent) and _same(res.vec["Yn"][p], inp["Yn"][p])   # and takes no step
    res, inp, sent = _launch("m33-n16-b17-pending-pass-fixed")         # it passes under fixed_iters: flag, then the step
    assert np.all(res.done[p] == 0) and np.all(res.status[p] & conv) and np.all(res.iters[p] == inp["it"])
    assert not _is_sentinel(res.vec["En"][p], sent)
    res, inp, sent = _launch("m33-n16-b17-pending-bump")               # it fails and mu is bumped: the step uses the new mu
    p = inp["flags"][:, FI["dpend"]] != 0
    mu0 = inp["state"][:, SI["mu"]]
    assert p.sum() >= 2 and np.all(res.done[p] == 0)
    ref = R.mspace_step(inp)
    stale = R.mspace_step(inp, model="stale_mu")                       # (the step with the mu from before the test)
    bi = ref["mask"]["bump_in"]
    assert bi.sum() >= 2 and np.all(res.mu[bi] >= mu0[bi] * np.float64(inp["rho"]))
    err_new = np.abs(res.vec["Yn"][bi] - ref["val"]["Yn"][bi]).max()
    err_old = np.abs(res.vec["Yn"][bi] - stale["val"]["Yn"][bi]).max()
    print(f"  pending-bump: Y_new against the step with the new mu {float(err_new):.3g}, with the stale mu {float(err_old):.3g}")
    assert err_old > 1e6 * err_new


@pytest.mark.parametrize("name", ["m33-n16-b17-pending-pass", "m33-n16-b17-pending-pass-fixed",
                                  "m33-n16-b17-pending-bump", "m33-n16-b17-pending", "m31-n16-b16-k5"])
def test_fin_finishes_only_the_pending_tests(name):
    """fin with realisations pending (each way the test can end), and with none: every buffer and every state field
    comes back bit for bit."""
    e = _Entry()
    inp = R.case(name)
    res = e.nms_host("fin", **_kw(inp))
    check_step(res, inp, name + " fin", e.SENTINEL, fin=True)
    if not (inp["flags"][:, FI["dpend"]] != 0).any():
        assert _same(res.state, inp["state"]) and np.array_equal(res.flags, inp["flags"])
        assert res.done_count == inp["done_count"]


# ------------------------------------------------------------------ 4: known answers
def test_zero_iterate_takes_the_zero_guard():
    """Y = M = 0 and a_z = 0: T = 0, g = 0, AX + M/mu = 0, so ArgMinY's zero guard gives Y_new = (B + mu) / (1 + mu),
    real, exactly; E_new = 0 shrinks to s = 0 with a_n' = mu."""
    e = _Entry()
    inp = dict(R.case("m33-n16-b17-k30"))
    b, m = inp["Yo"].shape
    z = np.zeros((b, m), np.complex128)
    st = inp["state"].copy()
    st[:, SI["naz"]] = 0.0
    st[:, SI["nbeta"]] = 0.0
    inp.update(Yo=z, Yn=z, M=z, state=st)
    res = e.nms_host("step", **_kw(inp))
    mu = st[:, SI["mu"]][:, None]
    want = (inp["B"] / 1.0 + mu) / (1.0 + mu)
    assert _same(res.vec["Yn"].real, want) and np.all(res.vec["Yn"].imag == 0.0)
    assert np.all(res.vec["En"] == 0) and np.all(res.vec["AEn"] == 0)
    assert np.all(res.naz == 0.0) and _same(res.nbeta, st[:, SI["mu"]]) and np.all(res.nep2 == 0.0)
    assert _same(res.dY2, res.nY2) and _same(res.nJM2, res.nY2) and np.all(res.nAX2 == 0.0)
    assert _same(res.vec["M"].real, -(want * mu)) and np.all(res.vec["M"].imag == 0.0)


def test_zero_x_init():
    e = _Entry()
    b, n, m = 3, 16, 33
    P0 = np.zeros((b, m), np.complex128)
    res = e.nms_host("init", batch=b, n=n, m=m, Xinit=np.zeros((b, n), np.complex128), P0=P0,
                     state=R.state_array(b, mu=4.0, nep2=7.0, naz=0.5, nx0=3.0))
    assert np.all(res.naz == 0.0) and np.all(res.nep2 == 0.0) and np.all(res.nx0 == 0.0) and np.all(res.na == 1.0)


# ------------------------------------------------------------------ 5: init and out
@pytest.mark.parametrize("m,n,b,scale", [(1, 4, 1, 1.0), (33, 16, 17, 5.0), (256, 64, 16, 1.0), (40, 300, 3, 0.1)])
def test_init(m, n, b, scale):
    e = _Entry()
    A, B, X0, Y0 = R.problem(50 + m, m, n, b)
    X0 = X0 * scale
    P0 = X0 @ A.T
    st = R.state_array(b, mu=4.0, last_res=np.inf, opt_obj=np.inf, nopt_a=9.0, ncur_a=9.0, nbeta=9.0, obj2=2.5)
    fl = np.zeros((b, len(R.FLAGS)), np.int32)
    fl[:, FI["dpend"]] = 1
    res = e.nms_host("init", batch=b, n=n, m=m, Xinit=X0, P0=P0, state=st, flags=fl)
    ref = R.mspace_init(X0, P0)
    label = f"init m{m} n{n} b{b}"
    all_ = np.ones(b, bool)
    s_n = ref["nx0"]                                                # a sum of n positive terms
    _within(res.nx0, ref["nx0"], s_n, all_, "init nx0", label)
    assert _same(res.nep2, res.nx0)
    nz = np.sqrt(ref["nx0"])
    s_az = np.where(nz > 1, 1 / nz * (s_n / (2 * nz) + nz) / nz + 1, 0)
    _within(res.naz, ref["naz"], s_az, all_, "init naz", label)
    assert np.array_equal(res.naz > 0, np.asarray(nz > 1))         # (both sides of the shrink are in the parameters)
    assert (res.naz > 0).any() == (m in (1, 33))
    assert np.all(res.vec["Eo"] == 0) and _same(res.vec["AEo"], P0)
    assert np.all(res.na == 1.0) and np.all(res.nbeta == 0.0) and np.all(res.nopt_a == 0.0) and np.all(res.ncur_a == 0.0)
    assert np.all(res.dpend == 0)
    for k in ("mu", "last_res", "opt_obj", "obj2"):                 # the rest of the control block is the caller's
        assert _same(getattr(res, k), st[:, SI[k]]), k
    _untouched(res, res.guards.keys(), label, e.SENTINEL)
    for k in ("Yn", "M", "En", "AEn", "optW", "optY", "curW", "Wsel", "V"):
        assert _is_sentinel(res.vec[k], e.SENTINEL), k


def test_out_selects_the_best_or_the_current_iterate():
    e = _Entry()
    b, n, m = 17, 16, 33
    rng = np.random.default_rng(5)
    cx = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    X0, optW, curW = cx(b, n), cx(b, m), cx(b, m)
    opt_obj = np.where(np.arange(b) % 3 == 1, np.inf, 0.25)
    opt_obj[4] = np.nan                                                # (not < inf: the current iterate)
    st = R.state_array(b, opt_obj=opt_obj, nopt_a=rng.standard_normal(b), ncur_a=rng.standard_normal(b))
    res = e.nms_host("out", batch=b, n=n, m=m, Xinit=X0, optW=optW, curW=curW, state=st)
    have = opt_obj < np.inf
    co = np.where(have, st[:, SI["nopt_a"]], st[:, SI["ncur_a"]])[:, None]
    assert _same(res.vec["V"].real, X0.real * co) and _same(res.vec["V"].imag, X0.imag * co)
    assert _same(res.vec["Wsel"], np.where(have[:, None], optW, curW))
    assert _same(res.vec["optW"], optW) and _same(res.vec["curW"], curW) and _same(res.state, st)
    _untouched(res, res.guards.keys(), "out", e.SENTINEL)


@pytest.mark.parametrize("name", list(R.RECORDED))
def test_out_of_an_iterate_recorded_past_init(name):
    """2, 5: a step past init (e != 0, a_n != 0, so c_v != a_z) with opt_obj = +inf records its iterate; out then
    selects it (the best one, or the current one of the realisation whose objective is NaN), and V + A^H Wsel, formed in
    longdouble here, is the n-space truth's X of that iteration."""
    e = _Entry()
    res, inp, sent = _launch(name)
    ref = R.mspace_step(inp)
    imp, cur = ref["mask"]["imp"], ref["mask"]["cur"]
    assert (imp | cur).all() and cur.sum() == (1 if name in R.NAN_B else 0)
    cv = inp["state"][:, SI["naz"]] - inp["state"][:, SI["nbeta"]] / inp["state"][:, SI["mu"]]
    assert np.all(np.abs(cv - inp["state"][:, SI["naz"]]) > 1e-3 * np.abs(cv)) and np.all(inp["Eo"] != 0)
    assert not _same(res.vec["optW"][imp], inp["optW"][imp]) and _same(res.vec["optY"][imp], res.vec["Yn"][imp])
    A, X0, truth = R.recorded_truth(name)
    b, n = X0.shape
    out = e.nms_host("out", batch=b, n=n, m=A.shape[0], Xinit=X0, optW=res.vec["optW"], curW=res.vec["curW"],
                     state=res.state)
    assert _same(out.vec["Wsel"], np.where(imp[:, None], res.vec["optW"], res.vec["curW"]))
    dev = R.recorded_deviation(out.vec["V"], out.vec["Wsel"], A, truth)
    bound = R.CHAIN_MULT * R.REC_DEV
    print(f"  {name}: V + A^H Wsel against the n-space X: {dev:.3g}, bound {bound:.3g} (ratio {dev / bound:.3g})")
    if dev / bound > WORST.get("recorded X", (0.0, ""))[0]:
        WORST["recorded X"] = (dev / bound, name)
    assert dev <= bound


# ------------------------------------------------------------------ 6: a chain from init against the n-space truth
@pytest.mark.parametrize("name", list(R.CHAINS))
def test_chain_of_five_steps_against_the_nspace_truth(name):
    e = _Entry()
    seed, m, n, b = R.CHAINS[name]
    par = {k: v for k, v in R.CHAIN_PAR.items() if k != "mu0"}
    ch = R.chain(seed, m, n, b, R.CHAIN_STEPS)
    A, B, X0, Y0 = R.problem(seed, m, n, b)
    G, K = R.LD.f64(ch.G), R.LD.f64(ch.K)
    P0 = R.LD.f64(R.LD.c(X0) @ R.LD.c(A).T)
    st = R.state_array(b, mu=R.CHAIN_PAR["mu0"], last_res=np.inf, opt_obj=np.inf)
    res = e.nms_host("init", batch=b, n=n, m=m, Xinit=X0, P0=P0, state=st)
    nxt = dict(Yo=Y0, M=np.zeros((b, m), np.complex128), Eo=res.vec["Eo"], AEo=res.vec["AEo"], state=res.state,
               flags=res.flags, done_count=0)
    steps = []
    for it in range(1, R.CHAIN_STEPS + 1):
        res = e.nms_host("step", batch=b, n=n, m=m, it=it, G=G, K=K, B=B, **par, **nxt)
        r = ch.rec[it]
        assert res.guard_ok and np.array_equal(res.dpend != 0, r["pending"]), (name, it)
        assert np.array_equal(res.iters, r["iters"]), (name, it)
        rc = np.where(res.dpend != 0, res.pd_rc, res.last_res)
        steps.append(dict(val=dict(Yn=res.vec["Yn"], nep2=res.nep2.copy(), naz=res.naz.copy(), res_comb=rc)))
        nxt = res.next()
    res = e.nms_host("fin", batch=b, n=n, m=m, it=R.CHAIN_STEPS, K=K, **par,
                     **{k: nxt[k] for k in ("Yo", "Yn", "state", "flags", "done_count")})
    last = ch.rec[R.CHAIN_STEPS]
    assert np.array_equal(res.iters, last["iters"]) and np.array_equal(res.status, last["status"])
    assert np.array_equal(res.done != 0, last["done"]) and np.all(res.dpend == 0)
    assert _same(res.mu, R.LD.f64(last["mu"])), (name, res.mu, last["mu"])
    out = e.nms_host("out", batch=b, n=n, m=m, Xinit=X0, optW=nxt["optW"], curW=nxt["curW"], state=res.state)
    X = out.vec["V"].astype(np.clongdouble) + out.vec["Wsel"].astype(np.clongdouble) @ np.conj(R.LD.c(A))
    dev = R.chain_deviation(steps, dict(X=X), ch)
    for k, v in dev.items():
        bound = R.CHAIN_MULT * R.CHAIN_DEV[k]
        print(f"  chain {name}: {k} deviation {v:.3g}, bound {bound:.3g} (ratio {v / bound:.3g})")
        if v / bound > WORST.get("chain " + k, (0.0, ""))[0]:
            WORST["chain " + k] = (v / bound, name)
    for k, v in dev.items():
        assert v <= R.CHAIN_MULT * R.CHAIN_DEV[k], (name, k, v)


# ------------------------------------------------------------------ 7: isolation
def test_nan_realisations_do_not_reach_their_block():
    """A NaN in B of one realisation and done realisations full of NaNs leave every other realisation of their blocks
    bit for bit as in the run without them; the done realisations' buffers are not written."""
    e = _Entry()
    name = "m40-n16-b33-k1-done"
    base, inp, sent = _launch(name)
    done = np.array(R.DONE_ROWS[name])
    bad = {k: np.array(inp[k], copy=True) for k in ("B", "Yo", "Yn", "M", "Eo", "AEo", "state")}
    for k in ("B", "Yo", "Yn", "M", "Eo", "AEo"):
        bad[k][done] = np.nan
    keep = [SI[k] for k in ("mu", "naz", "nbeta", "na", "nep2", "last_res", "opt_obj")]
    bad["state"][np.ix_(done, keep)] = np.nan
    jn = 7
    bad["B"][jn, 3] = np.nan
    res = e.nms_host("step", **_kw({**inp, **bad}))
    others = np.ones(33, bool)
    others[done] = False
    others[jn] = False
    for k in ("Yn", "M", "En", "AEn", "optW", "optY", "curW"):
        assert _same(res.vec[k][others], base.vec[k][others]), k
    assert _same(res.state[others], base.state[others]) and np.array_equal(res.flags[others], base.flags[others])
    assert np.isnan(res.obj2[jn]) and _same(res.vec["En"][jn], base.vec["En"][jn])
    for k in ("Yn", "M"):
        assert _same(res.vec[k][done], bad[k][done]), k
    for k in ("En", "AEn"):
        assert _is_sentinel(res.vec[k][done], sent), k
    assert _same(res.state[done], bad["state"][done]) and res.done_count == base.done_count
    _untouched(res, res.guards.keys(), name + " with NaNs", sent)


@pytest.mark.parametrize("j", [0, 15, 16, 23, 32])
def test_a_realisation_alone_equals_it_in_a_batch_of_33(j):
    e = _Entry()
    base, inp, sent = _launch("m40-n16-b33-k1-done")
    one = R.rows(inp, [j])
    one["done_count"] = 0
    res = e.nms_host("step", **_kw(one))
    for k in ("Yn", "M", "En", "AEn", "optW", "optY", "curW"):
        assert _same(res.vec[k][0], base.vec[k][j]), k
    assert _same(res.state[0], base.state[j]) and np.array_equal(res.flags[0], base.flags[j])
    _untouched(res, res.guards.keys(), f"row {j} alone", sent)
