"""CPU self-tests of tests/pl_ref.py: the restatements chained for two iterations equal the end-to-end oracle
(tfocs_oracle.tfocs_at_tracels); a perfect kernel (the restatement rounded to f64) passes the comparison of
tests/test_gpu_pl.py on every case of tests/pl_cases.py, with every decision margin holding; and twelve wrong-kernel
models each fail that same comparison on those same inputs."""
import numpy as np
import pytest

import pl_cases as C
import pl_ref as R
import tfocs_oracle as T


def _rounded(e, like):
    e = np.asarray(e)
    if e.dtype == R.LD:
        e = e.astype(np.float64)
        if like.dtype == np.complex128:
            e = e.view(np.complex128)
    return np.ascontiguousarray(e.reshape(like.shape)).astype(like.dtype)


def perfect(c):
    """What a correctly rounding kernel leaves behind on case c, and the reference's (arrays, state, tol)."""
    exp, S, tol = R.OPS[c.op](c.A, c.S, c.p)
    res = {k: np.array(v) for k, v in c.A.items()}
    for k, e in exp.items():
        res[k] = _rounded(e, c.A[k])
    return res, np.array(S), exp, S, tol


def verdict(c, res, state, exp, S, tol):
    return R.compare(res, state, exp, S, tol, c.A)


ALL = [c for f in C.GENERIC.values() for c in f()]


@pytest.mark.parametrize("c", ALL, ids=[c.id for c in ALL])
def test_a_perfect_kernel_passes_and_the_margins_hold(c):
    res, state, exp, S, tol = perfect(c)
    assert R.margins_hold(tol.get("margins", [])), tol.get("margins")
    assert verdict(c, res, state, exp, S, tol) <= 1.0
    # ... and one that touches a buffer it must not fails
    other = next(k for k in ("V1", "w", "K") if k not in exp)
    res[other] = res[other].copy()
    res[other].flat[-1] += 1.0
    assert verdict(c, res, state, exp, S, tol) == np.inf


# ---------------------------------------------------------------- the chain against the end-to-end oracle
def _step(op, A, S, p):
    exp, S2, _ = R.OPS[op](A, S, p)
    for k, e in exp.items():
        A[k] = _rounded(e, A[k])
    return S2


def _apply(A, X, out):
    Tl, _ = R.apply_a_T(dict(A, x=A[X]))
    Tc = _rounded(Tl, A["T"])
    A[out] = _rounded(R.diagform(A["R"], Tc, A["act"], A[out])[0], A[out])


@pytest.mark.parametrize("m,n", [(12, 16), (20, 9)])
def test_two_chained_iterations_equal_the_oracle(m, n):
    """From the zero start, two outer iterations of the restatements (with numpy's eigh between prox_in and
    assemble) against tfocs_at_tracels with maxIts = 2: (12, 16) in the reduced geometry (R = chol(Phi Phi^H)),
    (20, 9) with Q = I (R = Phi^H)."""
    rng = np.random.default_rng(m)
    Phi = (1j ** rng.integers(0, 4, (m, n))).astype(np.complex128)
    B = 2
    b = np.stack([np.abs(Phi @ (rng.standard_normal(n) + 1j * rng.standard_normal(n))) ** 2 / n for _ in range(B)])
    if m <= n:
        Rm = np.linalg.cholesky(Phi @ Phi.conj().T).conj().T
    else:
        Rm = Phi.conj().T.copy()
    d = Rm.shape[0]
    p = R.params(maxIts=2)
    A = {k: np.zeros(s, dt) for k, (s, dt) in C.shapes(B, m, d).items()}
    A.update(R=np.ascontiguousarray(Rm), RT=np.ascontiguousarray(Rm.T), bvec=b)
    S = _step("init", A, None, p)
    for _ in range(2):
        S = _step("outer_begin", A, S, p)
        for _inner in range(50):
            A["cnt"][:8] = 0
            S = _step("theta", A, S, p)
            if A["cnt"][0] == 0:
                break
            S = _step("make_y", A, S, p)
            if A["cnt"][1]:
                _apply(A, "y", "Aex")
            S = _step("set_ay", A, S, p)
            S = _step("grad", A, S, p)
            if A["cnt"][4]:
                S = _step("gy", A, S, p)
            S = _step("prox_in", A, S, p)
            for i in range(B):
                if A["act"][i]:
                    w, V = np.linalg.eigh(A["C"][i])
                    keep = np.where(w > A["tau"][i])[0][::-1]
                    A["V"][i][:len(keep)] = V[:, keep].T
                    A["lam"][i][:len(keep)] = w[keep]
                    A["misc"][i] = [len(keep), float(np.sum(w[keep] - A["tau"][i])), 0.0]
            S = _step("assemble", A, S, p)
            S = _step("zasm", A, S, p)
            S = _step("take_z", A, S, p)
            _apply(A, "z", "Az")
            S = _step("make_x", A, S, p)
            if A["cnt"][2]:
                _apply(A, "x", "Aex")
                S = _step("set_ax", A, S, p)
            S = _step("backtrack", A, S, p)
        S = _step("iterate", A, S, p)
    Rc = Rm.conj()
    for i in range(B):
        ref = T.tfocs_at_tracels(lambda X: np.real(np.sum(Rc * (X @ Rm), axis=0)), lambda g: (Rm * g[None, :]) @ Rm.conj().T,
                                 b[i], p["lam_reg"], np.zeros((d, d), np.complex128), maxIts=2, tol=p["tol"],
                                 restart=p["restart"])
        assert ref.niter == 2 == S[i, R.IX["n_iter"]] and S[i, R.IX["status"]] == 3
        assert np.abs(A["x"][i] - ref.x).max() <= 1e-12 * np.abs(ref.x).max()
        assert S[i, R.IX["L"]] == pytest.approx(ref.L, rel=1e-12)


# ---------------------------------------------------------------- wrong-kernel models
def _model(op, tag):
    c = C.find(op, tag)
    return (c,) + perfect(c)


def test_model_make_x_inner_product_against_x_old():
    c, res, state, exp, S, tol = _model("make_x", "d33")
    bad = R.make_x(dict(c.A, y=c.A["xo"]), c.S, c.p)[1]
    state[:, R.IX["dot_xy_g"]] = bad[:, R.IX["dot_xy_g"]]
    assert verdict(c, res, state, exp, S, tol) > 1.0


def _side_rows(c):
    return [b for b in range(c.batch) if c.A["act"][b] and c.A["misc"][b, 2] != 0.0]


def test_model_take_z_side_without_tau():
    c, res, state, exp, S, tol = _model("take_z", "d33-f0")
    for b in _side_rows(c):
        res["z"][b] += c.A["tau"][b] * np.eye(c.d)
    assert len(_side_rows(c)) >= 2 and verdict(c, res, state, exp, S, tol) > 1.0


def test_model_take_z_side_reads_the_other_tile_untransposed():
    """z(i1, j1) in tile (I, J), I < J, takes its W^H partner from wl[rr][cc] = W[32 J + rr][32 I + cc] instead of
    wl[cc][rr] = W[j1][i1] (and the mirrored tile likewise): visible only where there are two tiles (d > 32)."""
    c, res, state, exp, S, tol = _model("take_z", "d65-f1")
    d = c.d
    for b in _side_rows(c):
        W = c.A["zo"][b] - c.S[b, R.IX["step"]] * c.A["G"][b]
        z = res["z"][b]
        for i in range(d):
            for j in range(d):
                I, J = i // 32, j // 32
                if I == J:
                    continue
                pi, pj = 32 * J + i % 32, 32 * I + j % 32
                wrong = W[pi, pj] if pi < d and pj < d else 0.0
                z[i, j] += 0.5 * (np.conj(wrong) - np.conj(W[j, i]))
    assert verdict(c, res, state, exp, S, tol) > 1.0
    # at d <= 32 the same defect changes nothing: the d = 33 / 65 / 96 cases are what sees it
    assert C.find("take_z", "d31-f1").d == 31


def test_model_assemble_ignores_the_sign():
    c, res, state, exp, S, tol = _model("assemble", "d33-f0")
    for b in _side_rows(c):
        k = int(c.A["misc"][b, 0])
        res["P"][b][:, :k] = -res["P"][b][:, :k]
    assert any(c.A["misc"][b, 0] > 0 for b in _side_rows(c)) and verdict(c, res, state, exp, S, tol) > 1.0


def test_model_assemble_writes_unkept_columns_from_v():
    c, res, state, exp, S, tol = _model("assemble", "d64-f0")
    hit = 0
    for b in range(c.batch):
        k = int(c.A["misc"][b, 0])
        kw = min(c.d, 32 * ((k + 31) // 32))
        if c.A["act"][b] and k < kw:
            res["VT"][b][:, k:kw] = c.A["V"][b][k:kw, :].T
            hit += 1
    assert hit >= 2 and verdict(c, res, state, exp, S, tol) > 1.0


@pytest.mark.parametrize("d", [17, 23, 28, 33])
def test_model_outer_begin_drops_its_tail_loop(d):
    """Only the two-at-a-time loop (e + 256 < d^2; e += 512) runs: the entries it leaves keep their old contents.
    At d = 16 (d^2 = 256) the first loop copies nothing and at d = 32 everything, so the tails are what is tested."""
    c, res, state, exp, S, tol = _model("outer_begin", f"-d{d}")
    n2 = d * d
    copied = np.zeros(n2, bool)
    for t in range(256):
        e = t
        while e + 256 < n2:
            copied[e] = copied[e + 256] = True
            e += 512
    assert not copied.all()
    for b in range(c.batch):
        if not c.S[b, R.IX["done"]]:
            for k in ("xo", "zo"):
                res[k][b].reshape(-1)[~copied] = c.A[k][b].reshape(-1)[~copied]
    assert verdict(c, res, state, exp, S, tol) == np.inf


def test_model_iterate_restart_forgets_g_ay():
    c, res, state, exp, S, tol = _model("iterate", "restart-b7-m257")
    res["gAy"][1] = c.A["gAy"][1]
    assert verdict(c, res, state, exp, S, tol) == np.inf
    c, res, state, exp, S, tol = _model("iterate", "restart-b7-m257")
    state[2, R.IX["have_gAy"]] = 1          # have_gAx was 0: g_Ay must be recomputed
    assert verdict(c, res, state, exp, S, tol) == np.inf


def test_model_nonsimple_backtrack_does_not_store_g_ax():
    c, res, state, exp, S, tol = _model("backtrack", "nonsimple-b7-m40")
    res["gAx"] = c.A["gAx"].copy()
    assert verdict(c, res, state, exp, S, tol) == np.inf


def test_model_backtrack_divides_the_old_l_by_beta():
    c, res, state, exp, S, tol = _model("backtrack", "simple-b7-m40")
    L, loc = c.S[1, R.IX["L"]], state[1, R.IX["localL"]]
    assert state[1, R.IX["L"]] == pytest.approx(8 * L)
    state[1, R.IX["L"]] = max(loc, L / c.p["beta"])
    assert verdict(c, res, state, exp, S, tol) > 1.0


def test_model_theta_counter_test_is_strict():
    c, res, state, exp, S, tol = _model("theta", "reset3")
    ties = [b for b in range(c.batch) if res["act"][b] and state[b, R.IX["ycomp"]]
            and c.S[b, R.IX["cntr_Ay"]] == c.p["cntr_reset"]]
    assert len(ties) >= 3
    for b in ties:
        state[b, R.IX["need_Ay"]] = 0
        state[b, R.IX["cntr_Ay"]] = c.p["cntr_reset"] + 1.0
    res["cnt"][1] -= len(ties)
    assert verdict(c, res, state, exp, S, tol) == np.inf


def _chol_kernel(K, floor_only=False):
    """chol_kernel's arithmetic in f64 (row by row; a non-positive pivot is flagged and replaced by 1).  floor_only:
    the kernel as it was, sqrt(max(pivot, 1e-300)) on every pivot."""
    m = K.shape[0]
    Rm = np.zeros((m, m), np.complex128)
    bad = 0
    with np.errstate(all="ignore"):
        for j in range(m):
            s = K[j, j:] - Rm[:j, j].conj() @ Rm[:j, j:]
            djj = s[0].real
            bad |= not (djj > 0.0)
            piv = np.sqrt(max(djj, 1e-300)) if djj > 0.0 or floor_only else 1.0
            Rm[j, j:] = s / piv
            Rm[j, j] = piv
    return Rm, int(not bad)


def test_model_chol_reports_ok_on_an_indefinite_matrix():
    for c in C.chol_cases():
        Rm, ok = _chol_kernel(c.A["K"])
        if "indefinite" in c.id or "singular" in c.id:
            R.chol_expect_bad(Rm, ok)
            with pytest.raises(AssertionError):
                R.chol_expect_bad(Rm, 1)               # the model: ok reported on a matrix that is not definite
            if "indefinite" in c.id:                   # what test_gpu_pl found: 1e-150 pivots overflow two rows later
                with pytest.raises(AssertionError):
                    R.chol_expect_bad(*_chol_kernel(c.A["K"], floor_only=True))
        else:
            assert R.chol_check(c.A["K"], Rm, ok) <= 1.0
            Rm[0, -1] *= 1 + 1e-9 if c.m > 1 else 1 + 1e-6
            assert c.m == 1 or R.chol_check(c.A["K"], Rm, ok) > 1.0


def test_model_final_vec_without_the_factor_i():
    for c in C.final_vec_cases():
        w = R.final_vec_s(c.A, c.reduced)
        if c.reduced:
            w = np.stack([np.linalg.solve(c.A["R"].astype(np.complex128), w[b]) for b in range(c.batch)])
            if c.d <= 33:    # (numpy's solve is not the kernel's back substitution; small orders stay within gamma_d)
                assert R.final_vec_check(c.A, w, 1) <= 1.0
            w[0] *= 1 + 1e-9
            assert R.final_vec_check(c.A, w, 1) > 1.0
        else:
            assert R.final_vec_check(c.A, w, 0) == 0.0
            neg = c.A["lam"][:, 0] < 0
            assert neg.any()
            w[neg] = (w[neg] / 1j)
            with pytest.raises(AssertionError):
                R.final_vec_check(c.A, w, 0)
