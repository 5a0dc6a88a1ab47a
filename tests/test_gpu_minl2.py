"""GPU tests of the batched min-L2 ADMM (ace_minl2_*, csrc/ace_minl2.hip).

Target: the numpy restatement of tests/minl2_ref.py in long double.  A realisation "counts" when the oracle's float64,
long-double and row-permuted float64 runs agree with one another in iters, objcol and the mu schedule; at least 7 of
the 8 realisations of every shape and mode must count, and for those the kernel's iters, objcol and status are equal to
the target's and X, Y and opt_obj lie within max((m + n) u ||.||, 16 x spread), the rule of tests/test_gpu_gamp.py:
spread is the larger distance of the two float64 oracle runs from the long-double run, and norm and spread are those of
the quantity compared (in the per-column form the one column returned, not all r).

The per-column and r = 1 stages are chaotic over their full length (a relative 1e-15 perturbation of B
changes their iteration counts), so they are compared capped at 40 iterations, and at full length only invariants
are checked.  The row form is stable and is compared at full length.  With m <= n the per-column objectives are all at
rounding level and the best column is rounding noise: X is compared with the target's column at the kernel's own
objcol.  For the same reason the whole recovery is compared on its stable part (r_used, the first stage) and on the
median NMSE over 64 draws against the span of the oracle's own medians under 1e-15 perturbations of B.

Measured on the MI355X: DESIGN.md §4h has the err / bound table."""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import minl2_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

PARITY = [(n, m, mode) for n, m in R.SHAPES for mode in ("row", "col40", "r1_40") if (n, m, mode) != (20, 17, "col40")]
PARITY.append((5, 17, "col"))


def _run(c, **kw):
    from ace_amd import minl2
    return minl2.minl2_admm_host(c["A"], c["B"], c["X0"], scale_by_row=c["scale_by_row"], maxiter=c["maxiter"],
                                 want_xall=True, **kw)


def _dist(a, b):
    return float(np.sqrt(np.sum(np.abs(np.asarray(a, np.clongdouble) - np.asarray(b, np.clongdouble)) ** 2)))


@pytest.mark.parametrize("n,m,mode", PARITY, ids=[f"{n}x{m}-{mode}" for n, m, mode in PARITY])
def test_stage_parity(gpu, n, m, mode):
    from ace_amd import ACE_ST_CONVERGED
    c = R.stage_case(n, m, mode)
    assert sum(c["counts"]) >= 7, c["counts"]
    g = _run(c)
    worst = {"X": 0.0, "Y": 0.0, "Xall": 0.0, "opt_obj": 0.0}
    for b in range(R.NB):
        if not c["counts"][b]:
            continue
        ref, sp = c["ref"][b], c["spread"][b]
        assert g.iters[b] == ref["iters"], (b, g.iters[b], ref["iters"])
        assert g.objcol[b] == ref["objcol"], (b, g.objcol[b], ref["objcol"])
        assert int(g.status[b]) == (ACE_ST_CONVERGED if ref["converged"] else 0), (b, g.status[b])
        # X and Y as the stage returns them (all columns in the row form, the best column in the per-column form), each
        # against the bound of that same quantity; Xall (every column at the best iteration) against its own
        Xg, Yg = (g.X[b].T, g.Y[b].T) if c["scale_by_row"] else (g.X[b], g.Y[b])
        figs = {"X": (_dist(Xg, ref["X"]), R.bound(n, m, ref["X"], sp["X"])),
                "Y": (_dist(Yg, ref["Y"]), R.bound(n, m, ref["Y"], sp["Y"])),
                "Xall": (_dist(g.Xall[b].T, ref["Xall"]), R.bound(n, m, ref["Xall"], sp["Xall"])),
                "opt_obj": (abs(float(g.opt_obj[b] - ref["opt_obj"])), R.bound(n, m, ref["opt_obj"], sp["opt_obj"]))}
        assert np.array_equal(g.X[b], g.Xall[b] if c["scale_by_row"] else g.Xall[b, ref["objcol"]])
        for k, (err, bnd) in figs.items():
            worst[k] = max(worst[k], err / bnd)
    print(f"minl2 {n}x{m} {mode}: counting {sum(c['counts'])}/8, worst err / bound  " +
          "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (k, v)


def test_m_le_n_per_column(gpu):
    """Every column's objective is at rounding level: the kernel's column is compared with the target's SAME column."""
    n, m = 20, 17
    c = R.stage_case(n, m, "col40")
    g = _run(c)
    for b in range(R.NB):
        ref = c["ref"][b]
        j = int(g.objcol[b])
        assert g.iters[b] == ref["iters"] == 1 and 0 <= j < 20
        col = ref["Xall"][:, j]   # the bound of this column: its own norm, its own spread over the float64 runs
        spread = max(_dist(c["f64"][b]["Xall"][:, j], col), _dist(c["perm"][b]["Xall"][:, j], col))
        assert _dist(g.X[b], col) <= R.bound(n, m, col, spread), (b, j)
        assert g.opt_obj[b] <= 64 * m * R.U64 * np.linalg.norm(c["B"][b]), (b, g.opt_obj[b])


@pytest.mark.parametrize("n,m", [(16, 48), (64, 256)])
@pytest.mark.parametrize("mode", ["r1", "col"])
def test_full_length_chaotic_stages_keep_their_invariants(gpu, n, m, mode):
    """opt_obj is || |A X| - B || of the returned X.  The kernel's A X and numpy's are sums of n terms each; they differ
    by at most n u |a_i| |x| per entry in first order, i.e. by about n u ||A X|| in norm, and the objective moves by no
    more than that: the bound is (m + n) u max(||B||, ||A X||), the classical one."""
    from ace_amd import minl2, ACE_ST_CONVERGED
    sbr, cols, maxiter = R.MODES[mode]
    A, B, X0, _ = R.problem(n, m)
    X0 = X0 if cols is None else X0[:, :cols]
    g = minl2.minl2_admm_host(A, B, X0, scale_by_row=sbr, maxiter=maxiter)
    for b in range(R.NB):
        x = g.X[b].reshape(-1)
        ax = A @ x
        obj = np.linalg.norm(np.abs(ax) - B[b])
        assert abs(obj - g.opt_obj[b]) <= (m + n) * R.U64 * max(np.linalg.norm(B[b]), np.linalg.norm(ax)), (b, obj, g.opt_obj[b])
        assert 1 <= g.iters[b] <= maxiter
        conv = bool(int(g.status[b]) & ACE_ST_CONVERGED)
        assert int(g.status[b]) in (0, ACE_ST_CONVERGED)
        assert conv or g.iters[b] == maxiter      # a stage that left early passed the stop test
        assert np.isfinite(g.mu[b]) and g.mu[b] >= 1e-3


def test_the_limit_shape(gpu):
    """n = 1024, m = 4096 (the C-ABI's limits; the setup's largest Cholesky and the longest index arithmetic), three
    realisations of r = 20 columns with 20, 7 and 1 of them present, two iterations: the objective of the returned X is
    the one reported (the bound of the chaotic-stage test), and the second iteration's X satisfies the normal equations
    A^H (A X - S) = 0 of X = pinv(A) S to rounding, i.e. pinv(A) from the Cholesky factor is a pseudo-inverse."""
    from ace_amd import minl2
    n, m, r = 1024, 4096, 20
    rng = np.random.default_rng(77)
    A = np.exp(0.5j * np.pi * rng.integers(0, 4, (m, n))) / np.sqrt(n)
    x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
    B = np.abs(x @ A.T)
    X0 = rng.standard_normal((3, r, n)) + 1j * rng.standard_normal((3, r, n))
    rc = np.array([20, 7, 1], np.int32)
    g = minl2.minl2_admm_host(A, B, X0, scale_by_row=True, rcols=rc, maxiter=2, want_xall=True)
    assert (g.iters == 2).all() and (g.status == 0).all() and np.isfinite(g.X).all() and np.isfinite(g.Y).all()
    for b in range(3):
        X = g.X[b, :rc[b]].T
        assert not g.X[b, rc[b]:].any() and np.array_equal(g.X[b], g.Xall[b])
        AX = A @ X
        obj = np.linalg.norm(np.sqrt((np.abs(AX) ** 2).sum(axis=1)) - B[b])
        assert abs(obj - g.opt_obj[b]) <= (m + n) * R.U64 * max(np.linalg.norm(B[b]), np.linalg.norm(AX)), (b, obj, g.opt_obj[b])
        # X = pinv(A) S for some S: A X is the projection of S, so X = pinv(A) (A X) and G X = A^H (A X) with G = A^H A
        G = A.conj().T @ A
        res = np.linalg.norm(np.linalg.solve(G, A.conj().T @ AX) - X) / np.linalg.norm(X)
        assert res <= 1e-12, (b, res)


@pytest.mark.parametrize("r", [16, 1])
@pytest.mark.parametrize("sbr", [True, False])
def test_outputs_are_a_function_of_the_realisations_own_inputs(gpu, r, sbr):
    """Bit-identical alone, at another batch offset, through the host entry, with and without Xall; columns beyond
    rcols[b], filled with NaN, change nothing.  r = 16: one work-group per realisation; r = 1: 32 realisations each."""
    import torch
    from ace_amd import minl2
    n, m, nb = 16, 48, 40
    A, B8, X8, _ = R.problem(n, m)
    rng = np.random.default_rng(5)
    B = np.abs(B8[rng.integers(0, 8, nb)] * (1 + 0.01 * rng.standard_normal((nb, m))))
    X0 = (rng.standard_normal((nb, r, n)) + 1j * rng.standard_normal((nb, r, n)))
    kw = dict(scale_by_row=sbr, maxiter=40)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    full = minl2.minl2_admm_batch(up(A), up(B), up(X0), want_xall=True, **kw)
    host = minl2.minl2_admm_host(A, B, X0, want_xall=True, **kw)
    host0 = minl2.minl2_admm_host(A, B, X0, **kw)
    names = ("X", "Y", "iters", "objcol", "opt_obj", "mu", "Xall")
    F = {k: getattr(full, k).cpu().numpy() for k in names}
    for k in names:
        assert np.array_equal(F[k], getattr(host, k), equal_nan=True), k
        if k != "Xall":
            assert np.array_equal(F[k], getattr(host0, k), equal_nan=True), k
    assert np.array_equal(full.status.cpu().numpy().view(np.uint32), host.status)
    for b in (0, 7, 33, 39):   # alone (offset 0 of a batch of one) and at offset 2 of a batch of three
        one = minl2.minl2_admm_host(A, B[b:b + 1], X0[b:b + 1], want_xall=True, **kw)
        sel = [(b + 11) % nb, (b + 5) % nb, b]
        thr = minl2.minl2_admm_host(A, B[sel], X0[sel], want_xall=True, **kw)
        for k in names:
            assert np.array_equal(F[k][b], getattr(one, k)[0], equal_nan=True), (b, k)
            assert np.array_equal(F[k][b], getattr(thr, k)[2], equal_nan=True), (b, k)
    if r > 1:   # fewer columns: the rest of X0 is never read
        rc = rng.integers(1, r + 1, nb).astype(np.int32)
        rc[:3] = (r, 1, 3)
        Xz, Xn = X0.copy(), X0.copy()
        for b in range(nb):
            Xz[b, rc[b]:] = 0
            Xn[b, rc[b]:] = np.nan
        gz = minl2.minl2_admm_host(A, B, Xz, rcols=rc, want_xall=True, **kw)
        gn = minl2.minl2_admm_host(A, B, Xn, rcols=rc, want_xall=True, **kw)
        for k in names:
            assert np.array_equal(getattr(gz, k), getattr(gn, k)), k
        assert np.isfinite(gn.Xall).all() and np.isfinite(gn.opt_obj).all()
        for b in range(nb):   # ... and the realisation is the one with rcols[b] columns and nothing else
            one = minl2.minl2_admm_host(A, B[b:b + 1], X0[b:b + 1, :rc[b]], want_xall=True, **kw)
            assert np.array_equal(gn.Xall[b, :rc[b]], one.Xall[0]) and not gn.Xall[b, rc[b]:].any()
            assert gn.iters[b] == one.iters[0] and gn.opt_obj[b] == one.opt_obj[0] and gn.objcol[b] == one.objcol[0]


# ---------------------------------------------------------------- the whole recovery
N_REC, M_REC, DRAWS = 16, 64, 64


def _nmse(X, x):
    a = np.vdot(X, x) / np.vdot(X, X)
    return float(np.linalg.norm(a * X - x) ** 2 / np.linalg.norm(x) ** 2)


@pytest.fixture(scope="module")
def recovery():
    """64 draws at (16, 64): the float64 oracle on B and on three copies of B perturbed by a relative 1e-15."""
    A, B, _, x = R.problem(N_REC, M_REC, DRAWS, seed=31)
    tr = np.random.default_rng(4).permutation(M_REC)[:61].astype(np.int32)
    rng = np.random.default_rng(6)
    Bs = [B] + [B * (1 + 1e-15 * rng.standard_normal(B.shape)) for _ in range(3)]
    runs = [[R.infer_min_l2(A, Bk[b], tr) for b in range(DRAWS)] for Bk in Bs]
    return dict(A=A, B=B, x=x, tr=tr, runs=runs)


def _align(X, Xo):
    """X with each column turned by the unit phase that brings it onto Xo's (eigenvectors are defined up to one)."""
    ph = np.sum(np.conj(X) * Xo, axis=0)
    return X * (ph / np.abs(ph))[None, :]


def test_whole_recovery(gpu, recovery):
    from ace_amd import minl2, pipeline, ACE_ST_ROLLBACK
    A, B, x, tr, runs = (recovery[k] for k in ("A", "B", "x", "tr", "runs"))
    g = minl2.infer_min_l2_host(A, B, tr)
    base = runs[0]
    assert np.array_equal(g.r_used, [o[3]["r_used"] for o in base])
    assert np.array_equal(g.stage_iters[:, 0], [o[3]["stage_iters"][0] for o in base])   # the first stage is stable
    assert (g.stage_iters[:, 1] >= 1).all() and (g.stage_iters <= 500).all()
    for b in range(DRAWS):
        assert (g.stage_iters[b, 2] > 0) == (g.quality[b] > 0.6)
    # the stage-1 iterate: the library's spectral initialisation and row stage on the normalised train rows, against
    # the oracle's, column phases aligned; bound: the rule above with the spread of the perturbed oracle runs
    An = A / (np.linalg.norm(A) / np.sqrt(M_REC))
    Bn = B / np.linalg.norm(B, axis=1, keepdims=True)
    r = int(g.r_used.max())
    X0 = np.ascontiguousarray(np.transpose(pipeline.SpectralInitialize(An[tr], Bn[:, tr], r), (0, 2, 1)))   # [b][r][n]
    s1 = minl2.minl2_admm_host(An[tr], Bn[:, tr], X0, scale_by_row=True, rcols=g.r_used)
    assert np.array_equal(s1.iters, g.stage_iters[:, 0])
    worst = 0.0
    for b in range(DRAWS):
        rb = int(g.r_used[b])
        Xo = np.asarray(base[b][3]["stage1"]["X"], complex)
        spread = max(np.linalg.norm(_align(np.asarray(runs[k][b][3]["stage1"]["X"], complex), Xo) - Xo) for k in (1, 2, 3))
        err = np.linalg.norm(_align(s1.X[b, :rb].T, Xo) - Xo)
        worst = max(worst, err / R.bound(N_REC, M_REC - 3, Xo, spread))
    print(f"whole recovery: stage-1 iterate worst err / bound {worst:.3f}")
    assert worst <= 1.0
    # the median NMSE within the span of the oracle's four medians, widened 1.5 x each way (the summation order)
    med = [float(np.median([_nmse(o[0], x[b]) for b, o in enumerate(run)])) for run in runs]
    mine = float(np.median([_nmse(g.X[b], x[b]) for b in range(DRAWS)]))
    print("whole recovery: oracle medians " + " ".join(f"{v:.12e}" for v in med) + f"  kernel {mine:.12e}")
    lo, hi = min(med), max(med)
    assert lo - 1.5 * (hi - lo) <= mine <= hi + 1.5 * (hi - lo), (med, mine)
    rolled = (g.status & ACE_ST_ROLLBACK) != 0
    assert not rolled[g.quality <= 0.6].any()


def test_no_test_rows_means_no_refinement(gpu):
    from ace_amd import minl2
    A, B, _, _ = R.problem(16, 16)
    g = minl2.infer_min_l2_host(A, B)
    assert len(g.train_idx) == 16 and sorted(g.train_idx) == list(range(16))
    assert np.isnan(g.quality).all() and (g.stage_iters[:, 2] == 0).all()
    assert (g.stage_iters[:, :2] == 1).all()      # m_t <= n: both stages stop after one iteration
    assert np.isfinite(g.X).all()
    for b in range(R.NB):
        o = R.infer_min_l2(A, B[b], g.train_idx)
        assert np.isnan(o[2]) and g.r_used[b] == o[3]["r_used"]
    X, Y, q = minl2.inferMinL2(A, B[0])
    assert X.shape == (16, 1) and Y.shape == (16, 1) and np.isnan(q)


@pytest.mark.parametrize("r", [1, 2])
def test_the_floor_of_three_columns_can_exceed_r(gpu, r):
    """r < 3 with n, m_t >= 3: where the r leading eigenvalues hold 90 % of the spectrum the rule returns max(k, 3) = 3
    columns, more than r, and the reference takes a third eigenvector.  r_used and the first stage's count are the
    oracle's."""
    from ace_amd import minl2
    n, m = 3, 24
    A, B, _, x = R.problem(n, m)
    tr = np.random.default_rng(8).permutation(m)[:23].astype(np.int32)
    g = minl2.infer_min_l2_host(A, B, tr, r=r)
    ref = [R.infer_min_l2(A, B[b], tr, r=r) for b in range(R.NB)]
    Bp = B * (1 + 1e-15 * np.random.default_rng(9).standard_normal(B.shape))
    ref_p = [R.infer_min_l2(A, Bp[b], tr, r=r) for b in range(R.NB)]
    assert np.array_equal(g.r_used, [o[3]["r_used"] for o in ref])
    if r == 2:
        assert (g.r_used == 3).any() and (g.r_used == 2).any()      # both branches of the rule in one batch
    # the first stage's count where the oracle itself keeps it under a 1e-15 perturbation of B (one- and two-column
    # stages are not as stable as the r-column ones)
    stable = [b for b in range(R.NB) if ref[b][3]["stage_iters"][0] == ref_p[b][3]["stage_iters"][0]]
    assert len(stable) >= 6, stable
    for b in stable:
        assert g.stage_iters[b, 0] == ref[b][3]["stage_iters"][0], (b, g.stage_iters[b], ref[b][3]["stage_iters"])
    assert np.isfinite(g.X).all() and np.isfinite(g.quality).all()
    # one batch of mixed counts gives each realisation what it gets alone
    for b in (0, R.NB - 1):
        one = minl2.infer_min_l2_host(A, B[b:b + 1], tr, r=r)
        assert np.array_equal(one.X[0], g.X[b]) and np.array_equal(one.stage_iters[0], g.stage_iters[b])


def test_rank_deficient_A_is_unsupported(gpu):
    from ace_amd import minl2, AceError
    from ace_amd._lib import ACE_ERR_UNSUPPORTED
    A, B, X0, _ = R.problem(20, 17)
    A = A.copy()
    A[5] = A[2]   # a repeated row, m <= n
    with pytest.raises(AceError) as e:
        minl2.minl2_admm_host(A, B, X0, scale_by_row=True)
    assert e.value.code == ACE_ERR_UNSUPPORTED
    with pytest.raises(AceError) as e:
        minl2.infer_min_l2_host(A, B)
    assert e.value.code == ACE_ERR_UNSUPPORTED
