"""The PhaseLift step kernels (csrc/ace_phaselift.hip) one launch at a time through ace_pl_host, against the
restatements and derived bounds of tests/pl_ref.py (self-tested on the CPU by tests/test_pl_ref.py) on the inputs of
tests/pl_cases.py.

Every launch is handed every array of the entry; after it every buffer the operation does not write, every guard,
the rest of the eigensolver's scratch and the state block after the batch's must be bit for bit as they were (the
entry's guard_ok, and the comparison's own check of the arrays that went in).  Every decision taken from a rounded
quantity is first shown, on the reference alone, to sit at least four bounds away from its threshold
(pl_ref.margins_hold); the exactly representable ties (norm_dx == 0, xy_sq == 0, n_iter == maxIts,
cntr == cntr_reset, n_iter - restart_iter == restart, L >= Lexact, theta_old = Inf) are built exactly and must come
out exactly.  Each case prints its worst err / tol (pytest -s); the last test prints the worst per operation, which
DESIGN.md section 2.5c tabulates.
"""
import numpy as np
import pytest

import eig_ref as E
import pl_cases as C
import pl_ref as R
import tfocs_oracle as T

pytestmark = pytest.mark.gpu

WORST = {}


def _note(op, r):
    WORST[op] = max(WORST.get(op, 0.0), float(r))


def _host(c, op=None, **over):
    from ace_amd import plstep
    p = dict(c.p)
    kw = dict(c.A)
    kw.update(over)
    res = plstep.pl_host(op or c.op, batch=c.batch, m=c.m, d=c.d, reduced=c.reduced, state=c.S, **p, **kw)
    assert res.guard_ok, "a buffer the operation must not write, or a guard, changed"
    assert res.guards_hold()
    return res


def _run(c):
    exp, S, tol = R.OPS[c.op](c.A, c.S, c.p)
    if "margins" in tol:
        assert R.margins_hold(tol["margins"]), (c.id, tol["margins"])
    res = _host(c)
    worst = R.compare(res.arr, res.state, exp, S, tol, c.A)
    print(f"PLSTEP {c.id} worst err/tol {worst:.3g}")
    _note(c.op, worst)
    assert worst <= 1.0, (c.id, worst)
    return res


def _ids(cases):
    return [c.id for c in cases]


ELEMENTWISE = [c for op in ("init", "outer_begin", "theta", "make_y", "set_ay", "grad", "gy", "prox_in", "make_x",
                            "set_ax", "transpose", "outputs") for c in C.GENERIC[op]()]


@pytest.mark.parametrize("c", ELEMENTWISE, ids=_ids(ELEMENTWISE))
def test_step(gpu, c):
    """init, outer_begin (every copy-loop tail), theta (batch 257), make_y, set_Ay, grad, g_y, prox_in, make_x,
    set_Ax, transpose and outputs on mixed batches."""
    _run(c)


BACKTRACK = C.backtrack_cases()


@pytest.mark.parametrize("c", BACKTRACK, ids=_ids(BACKTRACK))
def test_backtrack(gpu, c):
    """xy_sq == 0; simple with localL <= L, finite growth, an overflowing quotient (localL = Inf), the forced reset
    and the flip to the non-simple form; non-simple with both outcomes (g_Ax stored, have_gAx set); a finite Lexact
    (L == Lexact and L > Lexact stop the growth, a larger localL is clamped)."""
    res = _run(c)
    if "nonsimple" in c.id:   # the branch no whole solve reaches: g_Ax = A_x - b where it ran, untouched elsewhere
        ran = (c.A["act"] == 1) & (c.S[:, R.IX["backtrack_simple"]] == 0) & (c.S[:, R.IX["xy_sq"]] != 0)
        assert ran.sum() >= 4
        assert np.array_equal(res.gAx[ran], (c.A["Ax"] - c.A["bvec"])[ran]) and (res.have_gAx[ran] == 1).all()
        assert np.array_equal(res.gAx[~ran], c.A["gAx"][~ran])


ITERATE = C.iterate_cases()


@pytest.mark.parametrize("c", ITERATE, ids=_ids(ITERATE))
def test_iterate(gpu, c):
    """Stop codes 0 to 4 and the NaN stop, the restart copies with have_gAx 0 and 1, a done realisation left
    untouched, cnt[8] incremented once per newly done realisation."""
    res = _run(c)
    newly = int(((res.done == 1) & (c.S[:, R.IX["done"]] == 0)).sum())
    assert res.cnt[8] == c.A["cnt"][8] + newly and newly >= 2
    if "stops" in c.id:
        assert res.status.tolist() == [1, 1, 0, 2, 3, 2, 0]
    else:
        assert res.status.tolist() == [4, 0, 0, 3, 3, 0, 2]
        for b, have in ((1, 1), (2, 0), (5, 1)):   # the restarts
            assert res.have_gAy[b] == have and res.have_gy[b] == 0 and np.isinf(res.theta[b])
            assert np.array_equal(res.gAy[b], c.A["gAx"][b]) and np.array_equal(res.y[b], c.A["x"][b])


# ---------------------------------------------------------------- the prox assembly: assemble, zasm, take_z
PROX = C.assemble_cases() + C.zasm_cases() + C.take_z_cases()


@pytest.mark.parametrize("c", PROX, ids=_ids(PROX))
def test_prox_steps_alone(gpu, c):
    """k in {0, 1, 31, 32, 33, d} on both sides of the prox; P and VT start as a large finite poison: assemble leaves
    the column tiles at or beyond 32 ceil(k / 32) as they were, and the klim GEMM never reads them."""
    res = _run(c)
    if c.op == "assemble":
        for b in range(c.batch):
            kw = min(c.d, 32 * ((int(c.A["misc"][b, 0]) + 31) // 32)) if c.A["act"][b] else 0
            assert (res.P[b][:, kw:] == C.POISON * (1 + 1j)).all() and (res.VT[b][:, kw:] == C.POISON * (1 - 1j)).all()
    if c.op == "zasm":
        assert np.isfinite(R.fv(res.Znew)).all() and np.abs(res.Znew).max() < 1e6


def _prox_problem(d, k, side, seed):
    """H = Q diag(w) Q^H in long double (tests/eig_ref.py's construction) with k eigenvalues above tau; the kept
    side's eigenvectors as the rows of V, rounded to f64."""
    rng = C.rng_of(61, d, k, seed)
    Q = E.unitary(d, seed)
    tau = 0.35
    w = np.concatenate([tau + rng.uniform(0.2, 2.0, k), tau - rng.uniform(0.2, 2.0, d - k)]).astype(R.LD)
    H = (Q * w[None, :]) @ Q.conj().T
    H = 0.5 * (H + H.conj().T)
    keep = np.arange(k, d) if side else np.arange(k)
    V = np.zeros((d, d), np.complex128)
    V[:len(keep)] = Q[:, keep].T.astype(np.complex128)
    lam = np.zeros(d)
    lam[:len(keep)] = w[keep].astype(np.float64)
    s = (w[:k] - tau)
    Z = (Q[:, :k] * s[None, :]) @ Q[:, :k].conj().T
    return H.astype(np.complex128), V, lam, len(keep), float(s.sum()), tau, 0.5 * (Z + Z.conj().T), Q, w


@pytest.mark.parametrize("d", [1, 2, 31, 32, 33, 65, 96])
def test_prox_chain_against_prox_trace(gpu, d):
    """assemble -> zasm -> take_z chained on one matrix per kept count and side, z against prox_trace of the same
    matrix from its constructed long-double decomposition (and tfocs_oracle.prox_trace against that, at eig_ref's
    1e-11 ||H||_F: the same operation).  Bound per entry: the three kernels' own bounds on the values that pass
    through them, plus the rounding of the inputs: 2u per entry of the two V factors, u |H| (side) --
        2 (k' + 8) u sum_q |s_q| (|v_qi|_1)(|v_qj|_1)  +  6 EPS (|H_ij| + tau [i == j])."""
    lam_reg, step = 0.5, 0.7
    ks = sorted({k for k in (0, 1, 31, 32, 33, d) if k <= d})
    combos = [(k, side) for k in ks for side in (0, 1)]
    B = len(combos)
    probs = [_prox_problem(d, k, side, 3 + i) for i, (k, side) in enumerate(combos)]
    c = C._case("assemble", "chain", B, 2, d, C.state(B, step=step), dict(lam_reg=lam_reg))
    A = c.A
    A["zo"] = np.stack([p[0] for p in probs])
    A["G"][:] = 0.0
    A["V"] = np.stack([p[1] for p in probs])
    A["lam"] = np.stack([p[2] for p in probs])
    A["misc"] = np.array([[p[3], p[4], side] for p, (k, side) in zip(probs, combos)], float)
    A["tau"] = np.full(B, probs[0][5])
    A["P"][:] = C.POISON
    A["VT"][:] = C.POISON
    r1 = _host(c, "assemble")
    r2 = _host(c, "zasm", P=r1.P, VT=r1.VT)
    r3 = _host(c, "take_z", Znew=r2.Znew)
    worst = 0.0
    for b, (p, (k, side)) in enumerate(zip(probs, combos)):
        H, V, lam, kk, ssum, tau, Zref, Q, w = p
        cz, Zo = T.prox_trace(lam_reg, H, tau / lam_reg)
        assert np.abs(Zo - Zref.astype(np.complex128)).max() <= E.TOL * np.linalg.norm(H)
        sq = np.abs(lam[:kk] - tau)
        v1 = np.abs(V[:kk].real) + np.abs(V[:kk].imag)
        tol = 2 * (kk + 8) * (R.EPS / 2) * ((v1 * sq[:, None]).T @ v1) + 6 * R.EPS * (np.abs(H) + tau * np.eye(d)) * side
        tol = np.repeat(tol, 2, axis=1) + np.finfo(float).tiny
        err = np.abs(R.fvl(Zref) - R.fv(r3.z[b]).astype(R.LD)).astype(np.float64)
        worst = max(worst, float((err / tol).max()))
        assert r1.C_z[b] == pytest.approx(lam_reg * ssum, rel=4 * R.EPS)
    print(f"PLSTEP prox-chain d={d} worst err/tol {worst:.3g}")
    _note("prox chain", worst)
    assert worst <= 1.0


# ---------------------------------------------------------------- apply_a: the RT GEMM, then pl_diagform
APPLY = C.apply_a_cases()


@pytest.mark.parametrize("c", APPLY, ids=_ids(APPLY))
def test_apply_a(gpu, c):
    """T = X R against the 3M bound; A(X) against the restated diagonal form of the T the GEMM left (so each kernel
    is held to its own bound); inactive realisations' rows of Aex untouched."""
    Tref, Ttol = R.apply_a_T(c.A)
    res = _host(c)
    rT = R.ratio(res.T, Tref, Ttol)
    exp, tol = R.diagform(c.A["R"], res.T, c.A["act"], c.A["Aex"])
    rA = R.ratio(res.Aex, exp, tol)
    for k, v in c.A.items():
        if k not in ("T", "Aex"):
            assert R.same(res.arr[k], v), k
    print(f"PLSTEP {c.id} worst err/tol T {rT:.3g} Aex {rA:.3g}")
    _note("apply_a (GEMM)", rT)
    _note("apply_a (diagform)", rA)
    assert rT <= 1.0 and rA <= 1.0


# ---------------------------------------------------------------- chol, final_vec
CHOL = C.chol_cases()


@pytest.mark.parametrize("c", CHOL, ids=_ids(CHOL))
def test_chol(gpu, c):
    res = _host(c)
    if "indefinite" in c.id or "singular" in c.id:
        R.chol_expect_bad(res.cholR, res.ok[0])
        return
    r = R.chol_check(c.A["K"], res.cholR, res.ok[0])
    print(f"PLSTEP {c.id} worst residual/bound {r:.3g}")
    _note("chol", r)
    assert r <= 1.0


FINAL = C.final_vec_cases()


@pytest.mark.parametrize("c", FINAL, ids=_ids(FINAL))
def test_final_vec(gpu, c):
    """lam > 0, = 0, < 0 in both geometries; d = 257 crosses the 256-thread stride of the back substitution."""
    res = _host(c)
    assert R.same(res.C, c.A["x"])                      # pl_final_in_kernel: a copy
    for k, v in c.A.items():
        if k not in ("C", "w"):
            assert R.same(res.arr[k], v), k
    r = R.final_vec_check(c.A, res.w, c.reduced)
    print(f"PLSTEP {c.id} worst residual/bound {r:.3g}")
    _note("final_vec", r)
    assert r <= 1.0


def test_zz_worst_ratios(gpu):
    """Prints the worst err / tol per operation over the cases above (run last)."""
    for op, r in WORST.items():
        print(f"PLSTEP-WORST {op}: {r:.3g}")
    assert all(r <= 1.0 for r in WORST.values())
