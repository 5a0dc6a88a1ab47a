"""The unit path's fused iteration kernels (gyk_kernel, gyf_kernel, msr_kernel, the fused epilogue of i8ah_kernel,
msr_ready_kernel, launch_i8_msp_optx; csrc/ace_i8gemm.hip) one launch at a time, against the references of
tests/unit_ref.py: (b) the kernels' specification in longdouble on exactly the f64 inputs of the launch, with the c, G
and K the setup made and a condition number per output, and (a) the n-space truth, one InferADMM A2only iteration with
Z explicit.

Everything goes through the test entry ace_unit_host (ace_amd.ustep), which builds the operators from the codebook as a
solve does, fills GykArgs, ZArgs, DualCtl and MsrArgs as admm_iterate_split does and makes one of the solve's launcher
calls.

Assertions (numbered as in DESIGN section 2.5d): 1 one step against (b), every vector elementwise and every sum, state
field and flag; 2 the same steps against (a) (gyk with apply_A folded in, gyf, ahf); 3 each rare branch, forced
through the state; 4 known answers without a reference; 5 an m-space run equals the chain of gyf launches bit for bit,
with its counters, for 8 and 4 waves, and its last state agrees with (b), with (a) and with the explicit Z0 + A^H S';
6 the readiness counts; 7 isolation.  Tolerances are TOL_MULT u kappa |value| plus the propagated int8 digit-plane
term of linop_ref (unit_ref: TOL_MULT is 8 x the f64 transcription's own worst ratio, floored at 1); every comparison
states err / tol (printed; the worst per output is printed when the module finishes and recorded in DESIGN).  The
inputs, their branches and their decision margins are shown on the reference alone by tests/test_unit_ref.py.

Measured on the MI355X (worst err / tol per output over the module; TOL_MULT = 48.8): g 0.25 (a caller's T at m = 256),
optx's opt_X 0.042, nAtY 0.032, Y' and opt_Y 0.020, M 0.017, nAX2 0.016, fs0 0.013, vbound 0.010, Z' 0.0099, every other
vector, sum and state field below 0.01; against the n-space truth AX 0.065, Y' 0.029, fs0 0.019, the rest below 0.01;
the last state of an m-space run below 0.004 against (b), 0.017 against (a), its fs0 0.0006 of the explicit bound.
128 cases in 13 s.
"""
import functools

import numpy as np
import pytest

import unit_ref as R

pytestmark = pytest.mark.gpu

WORST = {}      # output -> (worst err / tol seen, where)
SI = {k: i for i, k in enumerate(R.STATE)}
FI = {k: i for i, k in enumerate(R.FLAGS)}
PARAMS = ("it", "it_end", "maxiter", "fixed_iters", "tol_rel", "tol_abs", "rho", "lazy", "use_la", "use_ax", "yn_copy",
          "msp", "ctl", "room", "msp_fail_it", "waves", "done_count", "mspcount", "rank_one", "fl", "A", "B", "state",
          "flags")


class _Entry:
    """ace_amd.ustep with one rule added: a HIP error ends the session (nothing more is launched on a device that has
    reported a fault)."""

    def __init__(self):
        from ace_amd import ustep
        self._u = ustep
        self.SENTINEL = ustep.SENTINEL

    def unit_host(self, *a, **kw):
        from ace_amd import AceError
        try:
            return self._u.unit_host(*a, **kw)
        except AceError as e:
            if e.code == -3:
                pytest.exit(f"HIP error in ace_unit_host: {e}", returncode=3)
            raise


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module's tests: the worst err / tol per output over the comparisons that ran (pytest -s shows them).
    Every figure was asserted where it was measured; nothing is asserted here."""
    yield
    for k in sorted(WORST):
        print(f"  worst err/tol {k}: {WORST[k][0]:.3g} ({WORST[k][1]})")


def _bits(a):
    return np.ascontiguousarray(a).view(np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.all(_bits(a) == _bits(b)))


def _is_sentinel(x, s):
    return bool(np.all(np.ascontiguousarray(x).view(np.float64) == s))


def _kw(inp, **over):
    b, m = np.asarray(inp["B"]).shape
    kw = dict(batch=b, n=inp["n"], m=m, np_=inp["np"])
    for k in PARAMS:
        if k in inp:
            kw[k] = inp[k]
    for k in R.VEC_M + R.VEC_N:
        if inp.get(k) is not None:
            kw[k] = inp[k]
    if "q" in inp:
        kw["q"] = inp["q"]
    kw.update(over)
    return kw


def _call(e, inp, **over):
    """One launch of inp["op"]; returns the result and the inputs with the setup's own K, G and c in place."""
    res = e.unit_host(inp["op"], **_kw(inp, **over))
    return res, (R.with_ops(inp, res.K, res.G, res.c) if res.K is not None else inp)


def _record(ratios, label):
    for out, worst in ratios:
        print(f"  {label}: {out} err/tol {worst:.3g}")
        if worst > WORST.get(out, (0.0, ""))[0]:
            WORST[out] = (worst, label)


def _untouched(res, label, sentinel):
    for k, gd in res.guards.items():
        assert _is_sentinel(gd, sentinel), f"{label}: the guard after {k} was written"
    assert res.guard_ok, f"{label}: a control-block field or counter outside the launch's own was written"


def check_step(res, inp, label, sentinel):
    """Assertions 1, 3 and 7 on one launch: everything the launch wrote against (b), everything else at its input bits.
    The comparisons are unit_ref.compare_step, the function through which tests/test_unit_ref.py measures the
    wrong-step models."""
    _untouched(res, label, sentinel)
    ratios, broken, ref = R.compare_step(res, inp)
    _record(ratios, label)
    assert not broken, f"{label}: exact comparisons that do not hold: {broken}"
    bad = [(o, f"{w:.3g}") for o, w in ratios if not w <= 1.0]
    assert not bad, f"{label}: outside the tolerance (output, err/tol): {bad}"
    return ref


@functools.lru_cache(maxsize=None)
def _launch(name):
    e = _Entry()
    res, inp = _call(e, R.case(name))
    return res, inp, e.SENTINEL


# ------------------------------------------------------------------ 1, 3, 7: one step against the specification
@pytest.mark.parametrize("name", list(R.CASES))
def test_step_matches_the_specification(name):
    res, inp, sent = _launch(name)
    ref = check_step(res, inp, name, sent)
    print(f"  {name}: " + ", ".join(f"{k} {int(v.sum())}" for k, v in ref["mask"].items() if v.any()))


# ------------------------------------------------------------------ 2: the same steps against the n-space truth
TRUTH = ("gyk-", "gykL-", "gyf-", "gyfm-", "ahf-", "entry-", "defer-", "mixed-")


@pytest.mark.parametrize("name", [k for k in R.CASES if k.startswith(TRUTH)])
def test_step_matches_the_nspace_truth(name):
    """2: gyk with K Y and lazy (apply_A folded in, so Z is there; a caller's T has no n-space counterpart), gyf
    without and with m-space steps, and the stand-alone fused apply_AH."""
    res, inp, sent = _launch(name)
    ratios, ref, tr = R.compare_truth(res, inp)
    _record([("truth " + k, v) for k, v in ratios], name)
    print(f"  {name}: ||G - (I + K)^-1||_inf {tr['dG']:.3g}, kappa_inf(I + K) {tr['kappa']:.3g}")
    bad = [(o, f"{w:.3g}") for o, w in ratios if not w <= 1.0]
    assert not bad, f"{name}: outside the n-space bound (output, err/tol): {bad}"


# ------------------------------------------------------------------ 3: what the device's own flags say per branch
def test_each_rare_branch_on_the_device():
    conv = R.ST_CONVERGED
    role = lambda inp, *names: np.array([r in names for r in inp["roles"]])
    for tag in ("m17", "m121"):
        # a pending test that passes and stops: nothing of the realisation is written afterwards
        res, inp, sent = _launch(f"pend-stop-{tag}")
        p, fb, fk = role(inp, "pass_"), role(inp, "fail_b"), role(inp, "fail_k")
        q = (inp["it"] - 1) & 1
        assert p.sum() >= 2 and np.all(res.done[p] == 1) and np.all(res.status[p] & conv) and np.all(res.dpend[p] == 0)
        assert res.done_count - inp["done_count"] == p.sum()
        for k in (f"Y{1 - q}", "M", "AX", "Zb2" if inp["it"] & 1 else "Zb1", "X"):
            assert _same(res.vec[k][p], inp[k][p]), k
        mu0 = inp["state"][:, SI["mu"]]
        assert _same(res.mu[p], mu0[p]) and _same(res.obj2[p], inp["state"][p, SI["obj2"]])
        # ... that fails: mu rho exactly where res_comb grew, and T, g, Y' follow the new mu (early path)
        assert fb.sum() >= 2 and _same(res.mu[fb], mu0[fb] * np.float64(inp["rho"])) and _same(res.mu[fk], mu0[fk])
        assert np.all(res.dpend[fb | fk] == 0) and np.all(res.done[fb | fk] == 0)
        ref, stale = R.step(inp), R.step(inp, model="stale_mu")
        yn = f"Y{1 - q}"
        e_new = np.abs(res.vec[yn][fb] - ref["val"][yn][fb]).max()
        e_old = np.abs(res.vec[yn][fb] - stale["val"][yn][fb]).max()
        print(f"  pend-stop-{tag}: Y' against the step with the new mu {float(e_new):.3g}, the stale mu {float(e_old):.3g}")
        assert e_old > 1e6 * e_new
        # ... in the plain path (gyk_kernel without apply_A folded in)
        res2, inp2, _ = _launch(f"pend-plain-{tag}")
        e_new = np.abs(res2.vec[yn][fb] - R.step(inp2)["val"][yn][fb]).max()
        e_old = np.abs(res2.vec[yn][fb] - R.step(inp2, model="stale_mu")["val"][yn][fb]).max()
        assert e_old > 1e6 * e_new and _same(res2.mu[fb], mu0[fb] * np.float64(inp["rho"]))
        # ... under fixed_iters: flagged, not stopped, and the step runs
        res3, inp3, _ = _launch(f"pend-fixed-{tag}")
        assert np.all(res3.done == 0) and np.all(res3.status[p] & conv) and res3.done_count == inp3["done_count"]
        assert not _same(res3.vec[yn][p], inp3[yn][p])
        # deferred opt_Y: the buffer about to be overwritten is saved first, the other id is left alone
        res, inp, sent = _launch(f"defer-{tag}")
        this, that, fd = role(inp, "oy_this", "form_d"), role(inp, "oy_that"), role(inp, "form_d")
        assert _same(res.vec["optY"][this], inp[yn][this]) and np.all(res.optysrc[this] == 0)
        assert _same(res.vec["optY"][that], inp["optY"][that]) and np.all(res.optysrc[that] == 3 - (2 - q))
        # deferred opt_S: optsrc 4 + (it & 1) is saved from the S buffer this launch overwrites
        sn = f"S{inp['it'] & 1}"
        assert fd.sum() >= 2 and _same(res.vec["optS"][fd], inp[sn][fd]) and np.all(res.optsrc[fd] == 3)
        assert _same(res.vec["optS"][~fd], inp["optS"][~fd])
        # a mixed block: apply_A runs for the block, the others still take AX (bit for bit as without the cold one)
        res, inp, sent = _launch(f"mixed-block-{tag}")
        cold = role(inp, "cold")
        warm = dict(inp)
        fl = inp["flags"].copy()
        fl[cold, FI["done"]] = 1
        e = _Entry()
        resw, _ = _call(e, dict(warm, flags=fl))
        for k in (yn, "M", "AX", "Zb2" if inp["it"] & 1 else "Zb1"):
            assert _same(res.vec[k][~cold], resw.vec[k][~cold]), k
        assert _same(res.state[~cold], resw.state[~cold])
        # entry with room and with no room
        res, inp, sent = _launch(f"entry-{tag}")
        en, rf = role(inp, "enter"), role(inp, "refused")
        assert np.all(res.msp[en] == 1) and np.all(res.mzit[en] == inp["it"]) and np.all(res.msp_pad[en] == inp["it"])
        assert np.all(res.z0id[en] == (1 if inp["it"] & 1 else 2)) and res.mspcount == en.sum()
        assert np.all(res.msp[rf] == 0) and np.all(res.mzit[rf] == 0) and np.all(res.fzit[rf] == inp["it"])
        # msp_fail_it == it: the bound fails, the control writes nothing, the fused pass leaves the realisation alone
        res, inp, sent = _launch(f"fail-it-{tag}")
        tk = role(inp, "enter", "form")
        assert np.all(res.mzit[tk] == inp["it"]) and np.all(res.zit[tk] == inp["it"] - 1)
        assert _same(res.mu[tk], inp["state"][tk, SI["mu"]]) and _same(res.kfcum[tk], inp["state"][tk, SI["kfcum"]])
        # ctl = 0 and the last iteration: only the sums are written
        for nm in (f"ctl0-{tag}", f"fixup-{tag}"):
            res, inp, sent = _launch(nm)
            assert np.all(res.zit[tk] == inp["it"] - 1) and np.all(res.iters == inp["it"] - 1)
            assert np.all(res.mzit[tk] == inp["it"]) and not _same(res.fs0[tk], inp["state"][tk, SI["fs0"]])
        # converged: stops (and counts), or is only flagged under fixed_iters
        res, inp, sent = _launch(f"conv-{tag}")
        assert np.all(res.done == 1) and res.done_count == len(res.done) and np.all(res.status & conv)
        res, inp, sent = _launch(f"conv-fixed-{tag}")
        assert np.all(res.done == 0) and res.done_count == 0 and np.all(res.status & conv)


def test_gyf_returns_early_for_a_block_that_is_ahead():
    """3: every live realisation of block 0 has mzit >= it: all of its buffers and state stay at their input bits."""
    e = _Entry()
    inp0 = R.ahead_case()
    res, inp = _call(e, inp0)
    check_step(res, inp, "ahead", e.SENTINEL)
    for k in R.VEC_M + R.VEC_N:
        if inp.get(k) is not None:
            assert _same(res.vec[k][:16], inp[k][:16]), k
    assert _same(res.state[:16], inp["state"][:16]) and np.array_equal(res.flags[:16], inp["flags"][:16])
    assert not _same(res.state[16:], inp["state"][16:])


# ------------------------------------------------------------------ 4: known answers
def test_zero_iterate_takes_the_zero_guard():
    """Y = M = AX = 0 gives T = 0, g = 0 and AX + M/mu = 0: the zero guard, so Y' = (B + mu) / (1 + mu), real, exactly."""
    e = _Entry()
    inp = R.zero_guard_case()
    res, _ = _call(e, inp)
    q = (inp["it"] - 1) & 1
    mu = inp["state"][:, SI["mu"]][:, None]
    want = (inp["B"] / 1.0 + mu) / (1.0 + mu)
    yn = res.vec[f"Y{1 - q}"]
    assert _same(yn.real, want) and np.all(yn.imag == 0.0)
    assert np.all(res.vec["g"] == 0) and np.all(res.vec["AX"] == 0) and np.all(res.nAX2 == 0.0)
    assert _same(res.dY2, res.nY2) and _same(res.nJM2, res.nY2)


@pytest.mark.parametrize("m,n,b", [(17, 33, 17), (121, 256, 35)])
def test_unit_vector_g_returns_a_conjugated_row(m, n, b):
    """The fused apply_AH with g = e_i: W = c conj(A[i, :]) bit for bit, into X where there is no certificate and as
    Z' = 0 + W (fs0 = fs3) where there is one."""
    e = _Entry()
    inp = dict(R.build(15, m, n, b, "pmj", op="ahf", roles=("fused", "plain")))
    g = np.zeros((b, m), complex)
    rows = np.arange(b) % m
    g[np.arange(b), rows] = 1.0
    zc = "Zb1" if inp["it"] & 1 else "Zb2"
    zn = "Zb2" if inp["it"] & 1 else "Zb1"
    inp.update(g=g)
    inp[zc] = np.zeros((b, n), complex)
    res, _ = _call(e, inp)
    want = np.conj(inp["A"][rows])                       # c (P - jQ): A's entries are exactly +-c
    el = np.array([r == "fused" for r in inp["roles"]])
    assert _same(res.vec["X"][~el], want[~el]) and _same(res.vec[zn][el], want[el])
    assert _same(res.fs0[el], res.fs3[el]) and np.all(res.fzit[el] == inp["it"])
    _untouched(res, "unit g", e.SENTINEL)


@pytest.mark.parametrize("m,n,b", [(1, 1, 1), (17, 33, 17), (243, 64, 16)])
def test_optx_with_zero_opt_s_returns_z0(m, n, b):
    e = _Entry()
    inp = dict(R.build(16, m, n, b, "pmj1" if m == 1 else "pmj", op="optx", roles=("form",)))
    fl = inp["flags"].copy()
    src = np.array([3, 4, 5, 0, 1])[np.arange(b) % 5]
    fl[:, FI["optsrc"]] = src
    fl[:, FI["z0id"]] = 1 + (np.arange(b) // 5) % 2
    fl[:, FI["done"]] = np.arange(b) % 2                 # (done or not: the best iterate is still wanted)
    z = np.zeros((b, m), complex)
    inp.update(flags=fl, optS=z, S0=z, S1=z)
    res, _ = _call(e, inp)
    took = src >= 3
    want = np.where((fl[:, FI["z0id"]] == 1)[:, None], inp["Zb1"], inp["Zb2"])
    assert _same(res.vec["optX"][took], want[took]) and np.all(res.optsrc[took] == 0)
    assert _same(res.vec["optX"][~took], inp["optX"][~took]) and np.array_equal(res.optsrc[~took], src[~took])
    _untouched(res, "optx", e.SENTINEL)


@pytest.mark.parametrize("m,n,b", [(17, 33, 17), (256, 1024, 35)])
def test_optx_against_the_specification(m, n, b):
    e = _Entry()
    inp = dict(R.build(17, m, n, b, "pmj", op="optx", roles=("form",)))
    fl = inp["flags"].copy()
    fl[:, FI["optsrc"]] = np.array([3, 4, 5, 0, 2])[np.arange(b) % 5]
    fl[:, FI["z0id"]] = 1 + (np.arange(b) // 5) % 2
    inp.update(flags=fl)
    res, inp = _call(e, inp)
    ref = R.optx(inp)
    assert _same(res.vec["optS"][ref["gathered"]], R.F64.c(R.LD.f64(ref["optS"]))[ref["gathered"]])
    _record([("optx optX", R._ratio(res.vec["optX"], ref["optX"], ref["scale"], ref["extra"], ref["rows"]))], f"optx m{m}")
    assert R._ratio(res.vec["optX"], ref["optX"], ref["scale"], ref["extra"], ref["rows"]) <= 1.0
    assert np.array_equal(res.optsrc, ref["optsrc"]) and _same(res.vec["optX"][~ref["rows"]], inp["optX"][~ref["rows"]])
    _untouched(res, "optx", e.SENTINEL)


# ------------------------------------------------------------------ 5: an m-space run equals the chain of gyf launches
def _device_stepper(e):
    """unit_ref.run's per-iteration step made of one gyf launch (the masks read off the device's own state)."""
    def stepper(cur):
        it = cur["it"]
        res = e.unit_host("gyf", **_kw(cur))
        live = cur["flags"][:, FI["done"]] == 0
        with np.errstate(invalid="ignore"):
            imp = live & (np.sqrt(res.obj2) < cur["state"][:, SI["opt_obj"]])
        ok = live & (res.zit == it)
        val = {k: res.vec[k] for k in R.VEC_M + R.VEC_N}
        return dict(val=val, state={k: res.state[:, i] for k, i in SI.items()},
                    flags={k: res.flags[:, i] for k, i in FI.items()}, done_count=res.done_count, mspcount=res.mspcount,
                    mask=dict(run=live, ctl=ok, imp=imp, pendn=ok & (res.dpend != 0)), guard_ok=res.guard_ok)
    return stepper


RUNS = ([("m256-n64-b35", v, 8) for v in R.RUN_VARIANTS] + [("m256-n64-b16", v, 8) for v in ("end", "midstop")]
        + [("m256-n64-b35", v, 4) for v in ("end", "failbound", "pending", "midstop", "flush")] + [("m256-n64-b16", "end", 4)])


@pytest.mark.parametrize("shape,variant,waves", RUNS, ids=[f"{s}-{v}-w{w}" for s, v, w in RUNS])
def test_run_equals_the_chain_of_gyf_launches(shape, variant, waves):
    e = _Entry()
    inp0 = R.run_case(shape, variant)
    res, inp = _call(e, inp0, waves=waves)
    label = f"msr {shape} {variant} w{waves}"
    _untouched(res, label, e.SENTINEL)
    # the reference's run: the discrete outcome
    broken, ref = R.compare_run(res, inp)
    assert not broken, f"{label}: differs from the reference's run in {broken}"
    # the chain of gyf launches on the device, with the run's stop rules: bit for bit (unit_ref.compare_run_chain)
    ch = R.run(inp, stepper=_device_stepper(e))
    differs = R.compare_run_chain(res, inp, ch)
    assert not differs, f"{label}: differs from the chain of gyf launches in {differs}"
    ran = ch["ran"]
    # the last state of the run against (b), against (a), and fs0 against the explicit Z0 + A^H S'
    if waves == 8 and shape.endswith("b35") and variant in ("end", "failbound", "pending", "midstop"):
        it = ref["it_last"]
        assert it > inp["it"], label                       # several iterations inside the kernel
        q = (it - 1) & 1
        yn = f"Y{1 - q}"
        chref = R.run(dict(inp, it_end=it), stepper=_device_stepper(e))      # the device's state before iteration `it`
        cur = dict(inp, op="gyf", msp=1, it=it, state=chref["state"], flags=chref["flags"],
                   done_count=chref["done_count"], mspcount=chref["mspcount"], **chref["val"])
        so = f"S{(it + 1) & 1}"
        assert _same(res.vec[so][ran], cur[so][ran]), label
        cur[so] = np.where(ran[:, None], res.vec[so], cur[so])               # (the S the run wrote back)
        one = R.step(cur)
        rows = ran & one["mask"]["run"]
        assert rows.sum() >= 16, label
        ratios = [(k, R._ratio(res.vec[k], one["val"][k], one["scale"][k], 0.0, rows)) for k in (yn, "M", "AX")]
        ratios += [(k, R._ratio(res.state[:, SI[k]], one["state"][k], one["scale"][k], 0.0, rows))
                   for k in ("obj2", "nAX2", "nY2", "nJM2", "dY2", "fs0", "fs3")]
        _record([("run " + k, v) for k, v in ratios], label)
        assert all(v <= 1.0 for _, v in ratios), (label, ratios)
        truth, _, _ = R.compare_truth(res, cur, rows=rows)
        truth.append(("fs0 explicit", R.compare_run_fs0(res, inp, one, it, rows)))
        _record([("run truth " + k, v) for k, v in truth], label)
        assert all(v <= 1.0 for _, v in truth), (label, truth)


# ------------------------------------------------------------------ 6: the readiness counts
def test_ready_counts_on_a_hand_made_table():
    e = _Entry()
    b, it = 300, 12
    fl = R.flags_array(b, msp=1, mzit=it - 1, zit=it - 1)
    fl[3, FI["msp"]] = 0                      # not in the form
    fl[5, FI["dpend"]] = 1                    # a test pending
    fl[7, FI["mzit"]] = it - 2                # not settled through it - 1
    fl[9, FI["zit"]] = it - 2
    fl[11, FI["mzit"]] = it + 3               # taken past it by an earlier run: ready
    fl[13, FI["msp"]] = 0
    fl[13, FI["done"]] = 1                    # stopped: does not count
    fl[290, FI["msp"]] = 0                    # in the second 256-realisation group
    fl[291, FI["dpend"]] = 1
    res = e.unit_host("ready", batch=b, n=4, m=3, it=it, flags=fl)
    assert list(res.ready) == R.ready(fl, it) == [6, 2, 2]
    assert np.array_equal(res.flags, fl) and res.guard_ok
    res = e.unit_host("ready", batch=b, n=4, m=3, it=it, flags=R.flags_array(b, msp=1, mzit=it - 1, zit=it - 1))
    assert list(res.ready) == [0, 0, 0]


# ------------------------------------------------------------------ 7: isolation
@pytest.mark.parametrize("name", ["gyk-m121-n256-b35", "gyfm-m121-n256-b35"])
def test_nan_realisations_do_not_reach_their_block(name):
    """A NaN in B, an Inf in Y and a NaN in M of three realisations, and done realisations full of NaNs, leave every
    other realisation of their blocks bit for bit as in the run without them; the done rows are not written."""
    e = _Entry()
    base, inp, sent = _launch(name)
    b = len(inp["roles"])
    q = (inp["it"] - 1) & 1
    yo = f"Y{q}"
    done = np.array([r == "done" for r in inp["roles"]])
    bad = {k: np.array(inp[k], copy=True) for k in ("B", yo, "M", "AX")}
    for k in bad:
        bad[k][done] = np.nan
    live = np.nonzero(~done)[0]
    jb, jy, jm = live[1], live[7], live[-2]
    bad["B"][jb, 0] = np.nan
    bad[yo][jy, -1] = np.inf
    bad["M"][jm, 2] = np.nan
    cold = np.nonzero(np.array([r == "cold" for r in inp["roles"]]) & ~np.isin(np.arange(b), [jb, jy, jm]))[0]
    jv = cold[0]                              # apply_A's plane scale: a NaN bound on V makes the row's T NaN
    bad["state"] = inp["state"].copy()
    bad["state"][jv, SI["vbound"]] = np.nan
    res, _ = _call(e, {**inp, **bad})
    others = ~done
    others[[jb, jy, jm, jv]] = False
    for k in R.VEC_M + R.VEC_N:
        if inp.get(k) is not None and k not in ("B", yo):
            assert _same(res.vec[k][others], base.vec[k][others]), k
    assert _same(res.state[others], base.state[others]) and np.array_equal(res.flags[others], base.flags[others])
    assert np.isnan(res.obj2[jb]) and np.isnan(res.nY2[jy]) and np.isnan(res.nJM2[jm])
    assert np.all(np.isnan(res.vec["AX"][jv].view(np.float64))) and np.isnan(res.nAX2[jv]) and np.isnan(res.vbound[jv])
    if name.startswith("gyk-"):          # the plane scale of K Y' is NaN-sticky: the whole row and its dual terms
        assert np.all(np.isnan(res.vec[f"KY{1 - q}"][jy].view(np.float64))) and np.isnan(res.nAtY[jy])
    for k in (f"Y{1 - q}", "M", "AX"):
        assert _same(res.vec[k][done], {**inp, **bad}[k][done]), k
    assert _same(res.state[done], inp["state"][done])
    _untouched(res, name + " with NaNs", sent)


@pytest.mark.parametrize("name", ["ahf-m17-n33-b17", "ahf-m121-n256-b35"])
def test_nan_and_inf_in_g_stay_in_their_realisation(name):
    """The fused apply_AH with a NaN in g of a certified realisation and of one without a certificate, and an Inf in g
    of a third: the plane scale of A^H g is NaN-sticky (the whole row of Z' or W and fs0, fs3 are NaN), and every
    other realisation is bit for bit as without them."""
    e = _Entry()
    base, inp, sent = _launch(name)
    role = np.array(inp["roles"])
    zn = "Zb2" if inp["it"] & 1 else "Zb1"
    jn, jp, ji = np.nonzero(role == "fused")[0][1], np.nonzero(role == "plain")[0][1], np.nonzero(role == "fused")[0][2]
    g = np.array(inp["g"], copy=True)
    g[jn, 0] = np.nan
    g[jp, -1] = complex(0.0, np.nan)
    g[ji, 1] = np.inf
    res, _ = _call(e, dict(inp, g=g))
    others = np.ones(len(role), bool)
    others[[jn, jp, ji]] = False
    for k in R.VEC_M + R.VEC_N:
        if inp.get(k) is not None and k != "g":
            assert _same(res.vec[k][others], base.vec[k][others]), k
    assert _same(res.state[others], base.state[others]) and np.array_equal(res.flags[others], base.flags[others])
    for j in (jn, ji):
        assert np.all(np.isnan(res.vec[zn][j].view(np.float64))) and np.isnan(res.fs0[j]) and np.isnan(res.fs3[j])
        assert res.fzit[j] == inp["it"]
    assert np.all(np.isnan(res.vec["X"][jp].view(np.float64)))
    _untouched(res, name + " with NaN g", sent)


@pytest.mark.parametrize("j", [0, 15, 16, 23, 34])
@pytest.mark.parametrize("name", ["gyk-m121-n256-b35", "gyfm-m121-n256-b35"])
def test_a_realisation_alone_equals_it_in_its_batch(name, j):
    """Bit-identical alone (batch 1), whatever its position in a block and its block in the batch."""
    e = _Entry()
    base, inp, sent = _launch(name)
    one = dict(inp)
    for k in ("B", "state", "flags") + R.VEC_M + R.VEC_N:
        if inp.get(k) is not None:
            one[k] = np.ascontiguousarray(inp[k][j:j + 1])
    one["roles"] = inp["roles"][j:j + 1]
    res, _ = _call(e, one, done_count=0, mspcount=0)
    for k in R.VEC_M + R.VEC_N:
        if inp.get(k) is not None:
            assert _same(res.vec[k][0], base.vec[k][j]), k
    assert _same(res.state[0], base.state[j]) and np.array_equal(res.flags[0], base.flags[j])
    _untouched(res, f"{name} row {j} alone", sent)
