"""The kernels of csrc/ace_stage.hip on their own (ace_stage_host), against the longdouble references and derived
tolerances of tests/stage_ref.py.  Every test prints the worst err / tol of its op; each must stay at or below 1.
The cases' preconditions (decision margins, eigenvalue gaps, the reference inverse's residual) are asserted on the
CPU by tests/test_stage_ref.py."""
import math

import numpy as np
import pytest

import stage_ref as SR

pytestmark = pytest.mark.gpu

U = SR.U
SENT = -7.25e77


def _report(label, worst):
    print(f"  {label}: max err/tol {worst:.3g}")
    assert worst <= 1.0, (label, worst)


def _untouched(x):
    x = np.asarray(x)
    return bool(np.all(x.view(np.float64) == SENT)) if x.dtype.kind in "fc" else bool(np.all(x == 0x5A5A5A5A))


def _state(out, name):
    from ace_amd import stages
    return out["state_out"][:, stages.STATE.index(name)]


def _flag(out, name):
    from ace_amd import stages
    return out["flags_out"][:, stages.FLAGS.index(name)]


# ---------------------------------------------------------------- init_r / ystep_r
@pytest.mark.parametrize("mask", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("row", [True, False], ids=["row", "col"])
@pytest.mark.parametrize("case", SR.YCASES, ids=lambda c: "m%d-n%d-r%d-b%d" % c)
def test_init_r(gpu, case, row, mask):
    from ace_amd import stages
    m, n, r, batch = case
    d = SR.init_inputs(m, n, r, batch, 7, mask=mask)
    out = stages.stage_host("init_r", row_mode=int(row), batch=batch, n=n, m=m, r=r, mu0=1e-3, **d)
    ref, zero = SR.init_ref(d["X"], d["P0"], d["B"], row, d["mask"])
    print(f"\ninit_r {case} row={row} mask={mask}")
    _report("X", SR.err_over_tol(out["Xo"], *ref["X"]))
    _report("Y", SR.err_over_tol(out["Yo"], *ref["Y"]))
    _report("nB", SR.err_over_tol(_state(out, "nB"), *ref["nB"]))
    assert not out["Mo"].any() and not out["No"].any()
    assert (_state(out, "mu") == 1e-3).all() and np.isinf(_state(out, "last_res")).all()
    assert np.isinf(_state(out, "opt_obj")).all() and not out["flags_out"].any()
    if zero.any():   # the D == 0 rows: exact values, bit for bit
        want = np.broadcast_to(SR.init_zero_rows_f64(d["B"], r, row)[:, None, :], zero.shape)
        assert np.array_equal(out["Yo"][zero], want[zero].astype(np.complex128))
    if mask:
        assert not out["Yo"][np.broadcast_to(d["mask"][:, None, :] == 0, out["Yo"].shape)].any()
    if batch == 17:   # position invariance: the same inputs at batch index 0 and 16
        for k in ("Xo", "Yo", "Mo", "No", "state_out"):
            assert np.array_equal(out[k][0], out[k][16]), k


@pytest.mark.parametrize("mask", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("row", [True, False], ids=["row", "col"])
@pytest.mark.parametrize("case", SR.YCASES, ids=lambda c: "m%d-n%d-r%d-b%d" % c)
def test_ystep_r(gpu, case, row, mask):
    from ace_amd import stages
    m, n, r, batch = case
    d = SR.ystep_inputs(m, r, batch, 11, mask=mask)
    done = np.zeros(batch, np.int32)
    if batch >= 3:
        done[1] = 1
    mu = d.pop("mu")
    out = stages.stage_host("ystep_r", row_mode=int(row), batch=batch, m=m, r=r, state=stages.state_array(batch, mu=mu),
                            flags=stages.flags_array(batch, done=done, objcol=-1), **d)
    ref, dec = SR.ystep_ref(d["S"], d["g"], d["M"], d["B"], d["Y"], mu, row, d["mask"])
    live = done == 0
    print(f"\nystep_r {case} row={row} mask={mask}")
    _report("Y", SR.err_over_tol(out["Yo"][live], ref["Y"][0][live], ref["Y"][1][live]))
    _report("M", SR.err_over_tol(out["Mo"][live], ref["M"][0][live], ref["M"][1][live]))
    for k in ("obj2", "nAX2", "nY2", "nJM2", "dY2"):
        _report(k, SR.err_over_tol(_state(out, k)[live], ref[k][0][live], ref[k][1][live]))
    if not row:
        assert np.array_equal(_flag(out, "objcol")[live], dec[0][live])
    # the done realisation: Y_new keeps the sentinel, M and the control block are as they came
    if batch >= 3:
        assert _untouched(out["Yo"][1]) and np.array_equal(out["Mo"][1], d["M"][1])
        assert _state(out, "nAX2")[1] == 0 and _flag(out, "objcol")[1] == -1
    if mask:
        off = np.broadcast_to(d["mask"][:, None, :] == 0, out["Yo"].shape) & live[:, None, None]
        assert not out["Yo"][off].any() and np.array_equal(out["Mo"][off], d["M"][off])
    if batch == 17:
        for k in ("Yo", "Mo", "state_out"):
            assert np.array_equal(out[k][0], out[k][16]), k


def test_ystep_r_column_argmin_edges(gpu):
    """A NaN objective is skipped (also in column 0), and of two equal minimal columns the first wins."""
    from ace_amd import stages
    m, r = 37, 5
    d = SR.column_specials(m, r, 3)
    mu = d.pop("mu")
    d.pop("mask")
    out = stages.stage_host("ystep_r", row_mode=0, batch=3, m=m, r=r, state=stages.state_array(3, mu=mu), **d)
    ref, (col, margin) = SR.ystep_ref(d["S"], d["g"], d["M"], d["B"], d["Y"], mu, False)
    assert _flag(out, "objcol").tolist() == col.tolist() and col[2] == 1
    assert np.array_equal(out["Yo"][2, 1], out["Yo"][2, 2])          # the tie is exact on the GPU too
    print("\nystep_r column argmin edges")
    _report("Y", SR.err_over_tol(out["Yo"], *ref["Y"]))
    _report("obj2", SR.err_over_tol(_state(out, "obj2"), *ref["obj2"]))
    assert np.isnan(_state(out, "nAX2")[:2]).all() and np.isfinite(_state(out, "obj2")).all()


# ---------------------------------------------------------------- gram_rotate
@pytest.mark.parametrize("idx", range(len(SR.GRAM_CASES)), ids=["%s-n%d-r%d-b%d" % c for c in SR.GRAM_CASES])
def test_gram_rotate(gpu, idx):
    from ace_amd import stages
    c = SR.gram_case(idx)
    n, r, batch = c["n"], c["r"], c["batch"]
    out = stages.stage_host("gram_rotate", batch=batch, n=n, r=r, X=c["X"])
    assert not out["iout"].any()                                      # status stays 0
    worst = dict(a=0.0, b=0.0, c=0.0, d=0.0, null=0.0)
    for i in range(batch):
        st = SR.gram_stats(c["X"][i], out["Xo"][i], c["refs"][i], c["rank"])
        worst["a"] = max(worst["a"], st["a"] / SR.gram_tol_a(r))
        for k in "bcd":
            worst[k] = max(worst[k], st[k] / (SR.GRAM_MULT * SR.GRAM_ORACLE[k]))
        worst["null"] = max(worst["null"], st["null"])
        assert st["asc"], (i, "columns not in ascending order")
        if c["lam_exact"] is not None:   # the known answer: column norms^2 = n r s^2 (also the equal pair)
            d = np.sum(np.abs(out["Xo"][i]) ** 2, axis=1)
            tol = SR.GRAM_MULT * SR.GRAM_ORACLE["c"] * U * c["lam_exact"][-1]
            assert np.all(np.abs(d - c["lam_exact"]) <= tol), (d, c["lam_exact"])
    print(f"\ngram_rotate {SR.GRAM_CASES[idx]}")
    for k, v in worst.items():
        _report(f"({k})", v)
    if batch > 3:   # the batch cycles through three inputs: equal inputs give bit-identical outputs at any position
        assert np.array_equal(out["Xo"][0], out["Xo"][3]) and np.array_equal(out["Xo"][1], out["Xo"][16])


# ---------------------------------------------------------------- quality / part_quality
@pytest.mark.parametrize("n,mte,batch", [(1, 1, 3), (255, 13, 17), (257, 1, 1), (1024, 13, 3), (257, 0, 3)])
def test_quality(gpu, n, mte, batch):
    from ace_amd import stages
    rng = np.random.default_rng(5 + n + mte)
    A = rng.standard_normal((mte, n)) + 1j * rng.standard_normal((mte, n))
    X = rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))
    B = np.abs(rng.standard_normal((batch, mte))) + 0.1
    out = stages.stage_host("quality", batch=batch, n=n, count=mte, A=A, X=X, B=B)
    q, e = SR.quality_ref(A, X, B)
    print(f"\nquality n={n} mte={mte}")
    _report("q", SR.err_over_tol(out["qo"], q, e))
    if mte == 0:
        assert np.isnan(out["qo"]).all()


def test_quality_exactly_one_on_integer_data(gpu):
    from ace_amd import stages
    A, X, B = SR.exact_quality_inputs()
    out = stages.stage_host("quality", batch=3, n=A.shape[1], count=A.shape[0], A=A, X=X, B=B)
    assert (out["qo"] == 1.0).all()
    m = A.shape[0] + 2   # the same through part_quality: two train rows of junk in front
    rows = np.tile(np.r_[[m - 1, 0], np.arange(1, m - 1)].astype(np.int32), (3, 1))
    Af = np.vstack([7 * np.ones((1, A.shape[1])), A, 9j * np.ones((1, A.shape[1]))])
    Bf = np.hstack([np.full((3, 1), 2.0), B, np.full((3, 1), 3.0)])
    out = stages.stage_host("part_quality", batch=3, n=A.shape[1], m=m, mt=2, A=Af, X=X, B=Bf, rows=rows)
    assert (out["qo"] == 1.0).all()


@pytest.mark.parametrize("n,m,mte,batch", [(255, 40, 13, 17), (1024, 20, 1, 3), (1, 5, 4, 3)])
def test_part_quality(gpu, n, m, mte, batch):
    """B and A are read through rows[mt:], a different permutation for every realisation."""
    from ace_amd import stages
    rng = np.random.default_rng(50 + n)
    A = rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))
    X = rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))
    B = np.abs(rng.standard_normal((batch, m))) + 0.1
    rows, _ = SR.partition(m, m - mte, batch, 3)
    assert len({tuple(r) for r in rows[:, m - mte:]}) > 1 or batch == 1
    out = stages.stage_host("part_quality", batch=batch, n=n, m=m, mt=m - mte, A=A, X=X, B=B, rows=rows)
    te = rows[:, m - mte:]
    q, e = SR.quality_ref(A[te], X, np.take_along_axis(B, te.astype(np.int64), axis=1))
    print(f"\npart_quality n={n} m={m} mte={mte}")
    _report("q", SR.err_over_tol(out["qo"], q, e))


# ---------------------------------------------------------------- keep_best / finish / finalize_r: bit-exact
@pytest.mark.parametrize("first", [1, 0])
def test_keep_best(gpu, first):
    from ace_amd import stages
    rng = np.random.default_rng(13)
    n, m, b = 300, 257, 6
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)   # noqa: E731
    X, Y, Xm, Ym = c(b, n), c(b, m), c(b, n), c(b, m)
    q = np.array([0.9, 0.2, np.nan, 0.5, 0.5 * (1 + 2e-6), -2.0])      # better, not, NaN, equal, just better, below -1
    qmax = np.array([0.5, 0.5, 0.5, 0.5, 0.5, -1.0])
    with np.errstate(invalid="ignore"):   # the precondition: every comparison is 1e-6 away from equality, or exactly on it
        rel = np.abs(q - qmax) / np.abs(qmax)
    assert np.all(np.isnan(q) | (rel >= SR.MARGIN) | (q == qmax)) and q[3] == qmax[3]
    out = stages.stage_host("keep_best", batch=b, n=n, m=m, first=first, q=q, qmax=qmax, X=X, Y=Y, Xmax=Xm, Ymax=Ym)
    wq, wX, wY, better = SR.keep_best_f64(first, q, qmax, X, Y, Xm, Ym)
    assert better.tolist() == [True, False, False, False, True, False]
    assert np.array_equal(out["qo"], wq) and np.array_equal(out["Xo"], wX) and np.array_equal(out["Yo"], wY)
    assert np.array_equal(out["Xo"][2], X[2] if first else Xm[2])     # the NaN quality seeds X_max on the first restart only
    # no X_max yet (the buffers hold the sentinel): realisations that are not taken keep it
    out = stages.stage_host("keep_best", batch=b, n=n, m=m, first=first, q=q, qmax=qmax, X=X, Y=Y)
    for i in range(b):
        taken = better[i] or (first and np.isnan(q[i]))
        assert np.array_equal(out["Xo"][i], X[i]) if taken else _untouched(out["Xo"][i])


def test_finish(gpu):
    from ace_amd import stages
    from ace_amd._lib import ACE_ST_ROLLBACK
    d = SR.finish_cases()
    b, n, m, mt = 6, 37, 21, 17
    st_in = np.array([1, 1, 0, 4, 0, 0], np.int32)
    out = stages.stage_host("finish", batch=b, n=n, m=m, mt=mt, idst=st_in, **d)
    Xo, Yo, roll, _, _ = SR.finish_ref(d["q"], d["X"], d["Y"], d["Xmax"], d["Ymax"], d["anorm"], d["bnorm"])
    assert np.array_equal(out["iout"], st_in | np.where(roll, ACE_ST_ROLLBACK, 0))
    assert np.array_equal(out["Xo"], Xo) and np.array_equal(out["Yo"], Yo)      # x * (B_norm / A_norm), bit for bit
    assert roll[0] and not out["Yo"][0, mt:].any() and not roll[3]            # the zero tail; qlast == 0.6: no rollback


@pytest.mark.parametrize("bufs", [True, False], ids=["deferred-buffers", "no-buffers"])
@pytest.mark.parametrize("nc,r", [(1, 1), (1, 20), (20, 20)])
def test_finalize_r(gpu, nc, r, bufs):
    from ace_amd import stages
    from ace_amd._lib import ACE_ST_NO_OPT
    rng = np.random.default_rng(17)
    n, m, b = 257, 300, 10
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)   # noqa: E731
    optX, optY, Xc, Yc = c(b, nc, n), c(b, nc, m), c(b, r, n), c(b, r, m)
    Z1, Z2, Y1, Y2 = (c(b, nc, n), c(b, nc, n), c(b, nc, m), c(b, nc, m)) if bufs else (None,) * 4
    osrc = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 1], np.int32)
    oysrc = np.array([0, 1, 2, 1, 2, 0, 2, 0, 1, 2], np.int32)
    opt_obj = np.array([0.5] * 9 + [np.inf])                              # the last one never had a finite objective
    iters = np.arange(3, 3 + b, dtype=np.int32)
    status = np.array([0, 1, 0, 4, 1, 0, 0, 5, 0, 1], np.int32)
    mu = rng.uniform(1e-3, 1, b)
    out = stages.stage_host("finalize_r", batch=b, n=n, m=m, r=r, nc=nc, optX=optX, optY=optY, X=Xc, Y=Yc, Zb1=Z1,
                            Zb2=Z2, Yb1=Y1, Yb2=Y2, state=stages.state_array(b, mu=mu, opt_obj=opt_obj),
                            flags=stages.flags_array(b, iters=iters, status=status, optsrc=osrc, optysrc=oysrc))
    wX, wY, have = SR.finalize_f64(opt_obj, osrc, oysrc, optX, optY, Xc, Yc, nc, Z1, Z2, Y1, Y2)
    assert np.array_equal(out["Xo"], wX) and np.array_equal(out["Yo"], wY)
    if bufs:   # 1 and 2 select different buffers
        assert np.array_equal(out["Xo"][1], Z1[1]) and np.array_equal(out["Xo"][2], Z2[2])
        assert np.array_equal(out["Yo"][1], Y1[1]) and np.array_equal(out["Yo"][2], Y2[2])
    assert np.array_equal(out["iout"][:, 0], iters)
    assert np.array_equal(out["iout"][:, 1], status | np.where(have, 0, ACE_ST_NO_OPT))
    assert np.array_equal(out["qo"], mu)


# ---------------------------------------------------------------- part_geinv / part_gfix
GE_IDS = ["%s-m%d-n%d-te%d-r%d-b%d" % c for c in SR.GEINV_CASES]


@pytest.mark.parametrize("idx", range(len(SR.GEINV_CASES)), ids=GE_IDS)
def test_part_geinv(gpu, idx):
    from ace_amd import stages
    c = SR.geinv_case(idx)
    out = stages.stage_host("part_geinv", batch=c["batch"], m=c["m"], mt=c["mt"], G=c["G"], rows=c["rows"])
    assert not out["iout"].any()
    worst = 0.0
    for i in range(c["batch"] if c["te"] else 0):
        err = float(np.max(np.abs(out["Xo"][i].astype(np.clongdouble) - c["Xref"][i])))
        worst = max(worst, err / (SR.GJ_MULT * SR.GJ_RATIO * c["unit"][i]))
    print(f"\npart_geinv {SR.GEINV_CASES[idx]}")
    _report("geinv", worst)


@pytest.mark.parametrize("idx", range(len(SR.GEINV_CASES)), ids=GE_IDS)
def test_part_gfix(gpu, idx):
    """The kernel against the exact function of its inputs, and the Schur identity on the train rows."""
    from ace_amd import stages
    c = SR.geinv_case(idx)
    m, mt, te, r, batch = c["m"], c["mt"], c["te"], c["r"], c["batch"]
    gi = c["Xref"].astype(np.complex128)
    u = np.einsum("ij,brj->bri", c["G"], c["T"])
    done = np.zeros(batch, np.int32)
    if batch >= 3:
        done[batch - 1] = 1
    out = stages.stage_host("part_gfix", batch=batch, m=m, mt=mt, r=r, G=c["G"], geinv=gi, g=u, rows=c["rows"],
                            mask=c["mask"], flags=stages.flags_array(batch, done=done) if batch >= 3 else None)
    val, tol = SR.gfix_ref(c["G"], gi, u, c["rows"], mt)
    live = done == 0
    print(f"\npart_gfix {SR.GEINV_CASES[idx]}")
    _report("g", SR.err_over_tol(out["Yo"][live], val[live], tol[live]))
    if batch >= 3:
        assert np.array_equal(out["Yo"][batch - 1], u[batch - 1])         # the done realisation is left alone
    for i in np.flatnonzero(live):
        assert not out["Yo"][i][:, c["rows"][i][mt:]].any()
    worst = 0.0
    for i in range(min(int(live.sum()), 2)):
        want = SR.schur_direct(c["A"], c["T"][i], c["rows"][i], mt)
        err = np.linalg.norm((out["Yo"][i].astype(np.clongdouble) - want).astype(np.complex128), axis=1)
        t2 = np.linalg.norm(np.asarray(tol[i][..., 0], np.float64), axis=1)
        # (u = G T~ formed in f64 here: gamma_2m |G||T~| through (1 + ||W||) <= 2 sqrt(kappa))
        eu = 2 * math.sqrt(c["kappa"]) * SR.gam(2 * m + 2) * np.linalg.norm(np.abs(c["G"]) @ np.abs(c["T"][i]).T, axis=0)
        bound = SR.schur_tol(c["kappa"], m, te, c["T"][i], c["rows"][i], mt) + 2 * t2 + eu
        worst = max(worst, float(np.max(err / bound)))
    _report("Schur identity", worst)


def test_part_geinv_non_positive_pivot_sets_the_flag(gpu):
    from ace_amd import stages
    from ace_amd._lib import ACE_ST_EIG_NOCONV
    c = SR.geinv_case(2)
    G = c["G"].copy()
    bad = int(c["rows"][1][c["mt"]])                                      # the first test row of realisation 1
    G[bad, bad] = 0.0
    hit = np.array([bad in c["rows"][i][c["mt"]:] for i in range(c["batch"])])
    # (a zero pivot only where it is the first pivot or stays zero: realisation 1's first)
    out = stages.stage_host("part_geinv", batch=c["batch"], m=c["m"], mt=c["mt"], G=G, rows=c["rows"])
    assert out["iout"][1] == ACE_ST_EIG_NOCONV
    assert not out["iout"][~hit].any()


# ---------------------------------------------------------------- part_expand / part_compact, movers and norms
@pytest.mark.parametrize("m,mt,r,batch", [(300, 287, 20, 3), (257, 161, 1, 17), (5, 5, 2, 1)])
def test_part_expand_compact(gpu, m, mt, r, batch):
    from ace_amd import stages
    rng = np.random.default_rng(m)
    rows, _ = SR.partition(m, mt, batch, 5)
    src = rng.integers(-99, 99, (batch, r, mt)) + 1j * rng.integers(-99, 99, (batch, r, mt))
    full = stages.stage_host("part_expand", batch=batch, m=m, mt=mt, r=r, Y=src, rows=rows)["Yo"]
    want = np.zeros((batch, r, m), np.complex128)
    for i in range(batch):
        want[i][:, rows[i][:mt]] = src[i]
    assert np.array_equal(full, want)
    back = stages.stage_host("part_compact", batch=batch, m=m, mt=mt, r=r, Y=full, rows=rows)["Yo"]
    assert np.array_equal(back, src)


def test_norms(gpu):
    from ace_amd import stages
    rng = np.random.default_rng(23)
    for m, n in ((1, 1), (255, 31), (300, 257)):
        A = rng.integers(-3, 4, (m, n)) + 1j * rng.integers(-3, 4, (m, n))
        A[0, 0] = 1
        got = stages.stage_host("anorm", m=m, n=n, tol_abs=1e-8, A=A)["qo"][0]
        s = float(np.sum(np.abs(A) ** 2))                                 # integer: exact in any order
        assert got == np.sqrt(np.float64(s)) / np.sqrt(np.float64(m))
        B = rng.integers(0, 9, (3, m)).astype(np.float64)
        B[:, 0] = 1
        B[1] = 1e-12 * (B[1] > 0)                                         # below tol_abs: B_norm = 1
        out = stages.stage_host("bnorm", batch=3, m=m, tol_abs=1e-8, B=B)
        nb = np.sqrt(np.sum(B * B, axis=1))
        assert out["qo"][1] == 1.0 and out["qo"][0] == nb[0] and out["qo"][2] == nb[2]
        assert np.array_equal(out["Xo"], B / out["qo"][:, None])
    assert stages.stage_host("anorm", m=4, n=4, tol_abs=1e-8, A=1e-10 * np.ones((4, 4)))["qo"][0] == 1.0


def test_movers(gpu):
    from ace_amd import stages
    rng = np.random.default_rng(29)
    m, n, cnt, b = 300, 257, 17, 3
    A = rng.integers(-99, 99, (m, n)) + 1j * rng.integers(-99, 99, (m, n))
    idx = rng.permutation(m)[:cnt].astype(np.int32)
    an = np.array([4.0])
    got = stages.stage_host("gather_rows", m=m, n=n, count=cnt, A=A, idx=idx, anorm=an)["Xo"]
    assert np.array_equal(got, A[idx] * (np.float64(1.0) / an[0]))
    B = rng.integers(0, 99, (b, m)).astype(np.float64)
    assert np.array_equal(stages.stage_host("gather_b", batch=b, m=m, count=cnt, B=B, idx=idx)["qo"], B[:, idx])
    # gather then scatter with a permutation round-trips; rows that are not addressed keep the sentinel
    for ln in (1, 255, 514):
        src = rng.integers(-99, 99, (m, ln)).astype(np.float64)
        perm = rng.permutation(m).astype(np.int32)
        ga = stages.stage_host("move_rows", count=m, len=ln, m=m, scatter=0, src=src, idx=perm)["qo"]
        assert np.array_equal(ga, src[perm])
        assert np.array_equal(stages.stage_host("move_rows", count=m, len=ln, m=m, scatter=1, src=ga, idx=perm)["qo"], src)
        part = stages.stage_host("move_rows", count=cnt, len=ln, m=m, scatter=1, src=src[:cnt], idx=idx)["qo"]
        assert np.array_equal(part[idx], src[:cnt]) and _untouched(np.delete(part, idx, axis=0))
        bs = rng.integers(0, 255, (m, ln)).astype(np.uint8)
        gb = stages.stage_host("move_bytes", count=m, len=ln, m=m, scatter=0, bsrc=bs, idx=perm)["bout"]
        assert np.array_equal(gb, bs[perm])
        assert np.array_equal(stages.stage_host("move_bytes", count=m, len=ln, m=m, scatter=1, bsrc=gb, idx=perm)["bout"], bs)
    # put_col: plain and or-masked, with and without idx; more than one block of 256
    ld, col = 13, 5
    isrc = rng.integers(0, 1 << 20, m).astype(np.int32)
    dst = rng.integers(0, 1 << 20, (m, ld)).astype(np.int32)
    for use_idx in (False, True):
        for om in (0, 0x0F0F):
            k = cnt if use_idx else m - 3
            o = stages.stage_host("put_col", count=k, m=m, ld=ld, col=col, or_mask=om, isrc=isrc[:k],
                                  idx=idx if use_idx else None, idst=dst)["iout"]
            want = dst.copy()
            at = idx if use_idx else np.arange(k)
            want[at, col] = (dst[at, col] | (isrc[:k] & om)) if om else isrc[:k]
            assert np.array_equal(o, want)
    flag = (rng.uniform(size=m - 3) < 0.5).astype(np.uint8)
    o = stages.stage_host("flag_bits", count=m - 3, m=m, bit=128, bsrc=flag, idst=dst[:, 0].copy())["iout"]
    want = dst[:, 0].copy()
    want[:m - 3][flag != 0] |= 128
    assert np.array_equal(o, want)
    for ln in (0, 1, 255, 257):
        o = stages.stage_host("fill", len=ln, m=300, value=2.5)["qo"]
        assert (o[:ln] == 2.5).all() and _untouched(o[ln:])
