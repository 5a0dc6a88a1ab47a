"""CPU self-test of tests/stage_ref.py: the references against independent restatements (the numpy oracle's argmin_y,
normalize_rows and quality formula, numpy.linalg.inv / eigh, the Schur identity), the two measured constants, and every
precondition of every case of tests/test_gpu_stage.py, on the reference alone."""
import math

import numpy as np
import pytest

import ace_oracle as O
import stage_ref as SR

U = SR.U


def _c(v):
    """(re, im) longdouble array -> complex128."""
    v = np.asarray(v, np.float64)
    return v[..., 0] + 1j * v[..., 1]


@pytest.mark.parametrize("row", [True, False])
@pytest.mark.parametrize("case", SR.YCASES)
def test_init_reference_matches_the_oracle(case, row):
    m, n, r, batch = case
    d = SR.init_inputs(m, n, r, min(batch, 3), 7)
    ref, zero = SR.init_ref(d["X"], d["P0"], d["B"], row)
    for b in range(d["B"].shape[0]):
        AX, B, X = d["P0"][b].T.copy(), d["B"][b], d["X"][b].T.copy()        # m x r, n x r as the reference holds them
        if row:
            s = np.linalg.norm(B) / np.linalg.norm(AX)
            X, AX = X * s, AX * s
        else:
            s = np.linalg.norm(B) / np.linalg.norm(AX, axis=0)
            X, AX = X * s, AX * s
        Y = O.normalize_rows(AX, B, row)
        np.testing.assert_allclose(_c(ref["X"][0][b]), X.T, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(_c(ref["Y"][0][b]), Y.T, rtol=1e-11, atol=1e-300)
    if m >= 5:   # the zero rows are where they were put, and exact
        assert zero[:, :, 2].all() and zero[:, 0, 3].all() == (not row or r == 1)
        want = SR.init_zero_rows_f64(d["B"][:, 2], r, row)
        assert SR.err_over_tol(want, ref["Y"][0][:, 0, 2, 0], 2 * U * want) <= 1.0


@pytest.mark.parametrize("row", [True, False])
@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("case", SR.YCASES)
def test_ystep_reference_matches_the_oracle_and_its_decisions_have_margin(case, row, mask):
    m, n, r, batch = case
    d = SR.ystep_inputs(m, r, batch, 11, mask=mask)
    ref, dec = SR.ystep_ref(d["S"], d["g"], d["M"], d["B"], d["Y"], d["mu"], row, d["mask"])
    for b in range(min(batch, 3)):
        rows = np.flatnonzero(d["mask"][b]) if mask else np.arange(m)
        AX = (d["S"][b] - d["g"][b]).T[rows]
        Mb, mu, B = d["M"][b].T[rows], d["mu"][b], d["B"][b][rows]
        Y = O.argmin_y(AX, B, Mb.copy(), mu, row)
        got = _c(ref["Y"][0][b]).T
        np.testing.assert_allclose(got[rows], Y, rtol=1e-10, atol=1e-13)
        if mask:
            assert not got[np.setdiff1d(np.arange(m), rows)].any()
        np.testing.assert_allclose(_c(ref["M"][0][b]).T[rows], Mb + mu * (AX - Y), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(float(ref["nAX2"][0][b]), np.linalg.norm(AX) ** 2, rtol=1e-12)
        np.testing.assert_allclose(float(ref["nJM2"][0][b]), np.linalg.norm(AX - Y) ** 2, rtol=1e-10)
        if row:
            obj = np.linalg.norm(np.sqrt(np.sum(np.abs(AX) ** 2, axis=1)) - B)        # :345
            np.testing.assert_allclose(math.sqrt(float(ref["obj2"][0][b])), obj, rtol=1e-10)
        else:
            objs = np.sqrt(np.sum((np.abs(AX) - B[:, None]) ** 2, axis=0))               # :353
            assert dec[0][b] == int(np.argmin(objs))
            np.testing.assert_allclose(math.sqrt(float(ref["obj2"][0][b])), objs.min(), rtol=1e-10)
    if not row:
        assert (dec[1] >= SR.MARGIN).all(), dec[1]
    for k, (v, e) in ref.items():   # the bounds are small against the values: a derived tolerance, not a loose one
        v, e = np.asarray(v, np.float64), np.asarray(e, np.float64)
        big = np.abs(v) > 1e-3
        assert (e[big] <= 1e-9 * np.abs(v[big])).all() if k not in ("dY2",) else True, k


def test_column_specials_meet_their_preconditions():
    d = SR.column_specials(37, 5, 3)
    ref, (col, margin) = SR.ystep_ref(d["S"], d["g"], d["M"], d["B"], d["Y"], d["mu"], False)
    ax = d["S"] - d["g"]
    objs = np.sqrt(np.sum((np.abs(ax) - d["B"][:, None, :]) ** 2, axis=2))
    assert np.isnan(objs[0, 1]) and np.isnan(objs[1, 0]) and not np.isnan(np.delete(objs[0], 1)).any()
    assert col[0] == int(np.nanargmin(objs[0])) and col[0] != 1 and margin[0] >= SR.MARGIN
    assert col[1] == int(np.nanargmin(objs[1])) and col[1] != 0 and margin[1] >= SR.MARGIN
    assert col[2] == 1 and objs[2, 1] == objs[2, 2] and margin[2] == 0.0        # the exact tie: the first index wins
    assert (np.delete(objs[2], [1, 2]) >= objs[2, 1] * (1 + SR.MARGIN)).all()


def test_quality_reference_matches_the_oracle_formula():
    rng = np.random.default_rng(5)
    for n, mte in ((1, 1), (255, 13), (257, 1), (1024, 13)):
        A = rng.standard_normal((mte, n)) + 1j * rng.standard_normal((mte, n))
        X = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        B = np.abs(rng.standard_normal((3, mte))) + 0.1
        q, e = SR.quality_ref(A, X, B)
        for b in range(3):
            want = 1 - O._fro(np.abs(A @ X[b]).ravel() - B[b]) / O._fro(B[b])          # the oracle's :68
            assert abs(float(q[b]) - want) <= float(e[b]) + 4 * U * abs(want) + 1e-15 * n
            assert float(e[b]) <= 1e-9
    q, _ = SR.quality_ref(np.zeros((0, 4)), np.ones((2, 4)), np.zeros((2, 0)))
    assert np.isnan(q).all()                                                            # mte = 0: 0 / 0
    A, X, B = SR.exact_quality_inputs()
    q, e = SR.quality_ref(A, X, B)
    assert (q == 1).all()


def test_gj_restatement_inside_ratio_and_reference_residual():
    worst, worst_at = 0.0, None
    for idx, case in enumerate(SR.GEINV_CASES):
        c = SR.geinv_case(idx)
        assert (c["res"] <= 1e-17).all(), (case, c["res"].max())                        # the reference is accepted
        m, mt, te = c["m"], c["mt"], c["te"]
        for i in range(c["batch"] if te else 0):
            Gee = c["G"][np.ix_(c["rows"][i][mt:], c["rows"][i][mt:])]
            np.testing.assert_allclose(c["Xref"][i].astype(np.complex128), np.linalg.inv(Gee), rtol=0,
                                       atol=1e-9 * np.abs(c["Xref"][i]).max())
            err = float(np.max(np.abs(SR.gj_f64(Gee).astype(np.clongdouble) - c["Xref"][i])))
            ratio = err / c["unit"][i]
            if ratio > worst:
                worst, worst_at = ratio, (case, i)
    print(f"gj_f64: worst err / (te u kappa ||X||) = {worst:.4f} at {worst_at}")
    assert worst <= SR.GJ_RATIO


def test_schur_identity_and_gfix_reference():
    worst = 0.0
    for idx, case in enumerate(SR.GEINV_CASES):
        c = SR.geinv_case(idx)
        m, mt, te, r = c["m"], c["mt"], c["te"], c["r"]
        nb = min(c["batch"], 2)
        u = np.einsum("ij,brj->bri", c["G"].astype(np.clongdouble), c["T"][:nb].astype(np.clongdouble))
        u64 = u.astype(np.complex128)
        # the exact function on the f64 inputs the kernel gets (u and geinv rounded to f64)
        gi64 = c["Xref"][:nb].astype(np.complex128)
        val, tol = SR.gfix_ref(c["G"], gi64, u64, c["rows"][:nb], mt)
        g = val[..., 0] + 1j * val[..., 1]
        for i in range(nb):
            assert not g[i][:, c["rows"][i][mt:]].any()
            want = SR.schur_direct(c["A"], c["T"][i], c["rows"][i], mt)
            err = np.linalg.norm((g[i] - want).astype(np.complex128), axis=1)
            # u was rounded to f64 as well: u ||u|| through (1 + ||W||) <= 2 sqrt(kappa)
            bound = SR.schur_tol(c["kappa"], m, te, c["T"][i], c["rows"][i], mt) + \
                2 * math.sqrt(c["kappa"]) * U * np.linalg.norm(u64[i], axis=1)
            worst = max(worst, float(np.max(err / bound)))
            # T~ on the test rows does not matter: change it, the train rows stay within the same bound
            T2 = c["T"][i].copy()
            T2[:, c["rows"][i][mt:]] *= -3.0
            u2 = (c["G"].astype(np.clongdouble) @ T2.astype(np.clongdouble).T).T.astype(np.complex128)
            v2, _ = SR.gfix_ref(c["G"], gi64[i:i + 1], u2[None], c["rows"][i:i + 1], mt)
            g2 = v2[0, ..., 0] + 1j * v2[0, ..., 1]
            b2 = SR.schur_tol(c["kappa"], m, te, T2, c["rows"][i], mt) + \
                2 * math.sqrt(c["kappa"]) * U * np.linalg.norm(u2, axis=1)
            assert (np.linalg.norm((g2 - want).astype(np.complex128), axis=1) <= b2).all(), case
        assert float(np.max(np.asarray(tol, np.float64))) <= 1e-10
    print(f"Schur identity: worst err / bound = {worst:.3f}")
    assert worst <= 1.0


def test_gram_oracle_inside_ratios_and_preconditions():
    worst = {"orth": 0.0, "b": 0.0, "c": 0.0, "d": 0.0}
    for idx, case in enumerate(SR.GRAM_CASES):
        c = SR.gram_case(idx)
        kind, n, r, batch = case
        for i in range(min(batch, 3)):
            ref = c["refs"][i]
            Xo, V = SR.gram_oracle(c["X"][i])
            w = np.linalg.eigvalsh(c["X"][i].conj() @ c["X"][i].T)
            np.testing.assert_allclose(np.asarray(ref["lam"], np.float64), w, rtol=0, atol=1e-10 * max(ref["normH"], 1))
            st = SR.gram_stats(c["X"][i], Xo, ref, c["rank"])
            worst["orth"] = max(worst["orth"], float(np.linalg.norm(V @ V.conj().T - np.eye(r))) / (U * r))
            assert st["a"] <= SR.gram_tol_a(r), (case, st)
            for k in "bcd":
                worst[k] = max(worst[k], st[k])
            if c["rank"] is None:
                assert st["asc"]
                if kind == "full":
                    assert (ref["relgap"] >= SR.GAP).all(), (case, ref["relgap"].min())   # (c), (d) apply to every column
            else:
                assert st["null"] <= 1.0, (case, st)
            if kind == "hadamard":
                np.testing.assert_array_equal(np.asarray(ref["lam"], np.float64), c["lam_exact"])
                assert (ref["relgap"] < SR.GAP).sum() == 2                              # the equal pair, and only it
    print("gram oracle: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= SR.GRAM_ORACLE[k], (k, v)


def test_finish_decisions_have_margin():
    d = SR.finish_cases()
    Xo, Yo, roll, mq, ms = SR.finish_ref(d["q"], d["X"], d["Y"], d["Xmax"], d["Ymax"], d["anorm"], d["bnorm"])
    assert roll.tolist() == [True, False, False, False, False, False]
    assert (ms >= SR.MARGIN).all() and (np.delete(mq, 3) >= SR.MARGIN).all() and d["q"][3] == 0.6
    assert not Yo[0, 17:].any() and Yo[1, 17:].all()
    # the oracle's similarity (:93)
    for i in range(6):
        sim = abs(np.vdot(d["Xmax"][i], d["X"][i])) / np.linalg.norm(d["Xmax"][i]) / np.linalg.norm(d["X"][i])
        assert (sim < 0.6) == (i not in (1, 4))
