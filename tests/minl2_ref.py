"""numpy restatement of ADMM_v2/inferMinL2.m (lambda = 0), the oracle of the min-L2 tests.

Dtype-parametrised: ``np.float64`` runs MATLAB's arithmetic (``np.linalg.pinv``), ``np.longdouble`` the same
statements in extended precision (pinv by a twice-orthogonalised Gram-Schmidt QR, since LAPACK has no long double).
The spectral initialisation needs ``eig`` and exists in float64 only; its result is cast.

``infer_admm`` is InferADMM (:229-326) and returns everything a test compares: the best iterate (all columns and the
one returned), iters, objcol, opt_obj, mu and the mu schedule.  ``infer_min_l2`` is the whole file with the partition
passed in (0-based train rows; the test rows are the sorted complement).
"""
import numpy as np


def ctype(dtype):
    return np.clongdouble if np.dtype(dtype) == np.dtype(np.longdouble) else np.complex128


def _qr_mgs2(A):
    """A = Q R by modified Gram-Schmidt, each column orthogonalised twice; A tall with full column rank."""
    m, n = A.shape
    Q = A.copy()
    R = np.zeros((n, n), A.dtype)
    for j in range(n):
        for _ in range(2):
            for i in range(j):
                h = np.vdot(Q[:, i], Q[:, j])
                R[i, j] += h
                Q[:, j] = Q[:, j] - h * Q[:, i]
        R[j, j] = np.sqrt(np.vdot(Q[:, j], Q[:, j]).real)
        Q[:, j] = Q[:, j] / R[j, j]
    return Q, R


def pinv(A, dtype=np.float64):
    """pinv of a full-rank A in ``dtype``."""
    if np.dtype(dtype) == np.dtype(np.float64):
        return np.linalg.pinv(np.asarray(A, np.complex128))
    A = np.asarray(A, ctype(dtype))
    if A.shape[0] < A.shape[1]:
        return pinv(A.conj().T, dtype).conj().T
    Q, R = _qr_mgs2(A)
    n = R.shape[0]
    Ri = np.zeros_like(R)   # R^-1 by back substitution on the identity
    for j in range(n - 1, -1, -1):
        e = np.zeros(n, R.dtype)
        e[j] = 1
        Ri[j] = (e - R[j, j + 1:] @ Ri[j + 1:]) / R[j, j]
    return Ri @ Q.conj().T


def _norm(x):
    return np.sqrt(np.sum(np.abs(x) ** 2))


def normalize_rows(Y, B, scale_by_row):
    Y = Y.copy()
    r = Y.shape[1]
    if scale_by_row:
        D = np.sqrt(np.sum(np.abs(Y) ** 2, axis=1))
        z = D == 0
        Y[z, :] = 1 / np.sqrt(Y.real.dtype.type(r))
        D[z] = 1
        return Y * (B / D)[:, None]
    D = np.abs(Y)
    z = D == 0
    Y[z] = 1
    D[z] = 1
    return Y * (B[:, None] / D)


def argmin_y(AX, B, M, mu, scale_by_row):
    Y = AX + M / mu
    r = Y.shape[1]
    if scale_by_row:
        D = np.sqrt(np.sum(np.abs(Y) ** 2, axis=1))
        z = D == 0
        Y[z, :] = 1 / np.sqrt(Y.real.dtype.type(r))
        D[z] = 1
        return Y * ((B / D + mu) / (1 + mu))[:, None]
    D = np.abs(Y)
    z = D == 0
    Y[z] = 1
    D[z] = 1
    return Y * ((B[:, None] / D + mu) / (1 + mu))


def _first_min_skipping_nan(v):
    """MATLAB's [obj, j] = min(v): NaN skipped, first index; all NaN gives (NaN, 0)."""
    ok = ~np.isnan(v)
    if not ok.any():
        return v[0], 0
    j = int(np.flatnonzero(ok)[np.argmin(v[ok])])
    return v[j], j


def infer_admm(A, B, X0, scale_by_row, dtype=np.float64, maxiter=500, tol_rel=1e-4, tol_abs=1e-8, U=None, mu0=1e-3,
               rho=1.03):
    """InferADMM (:229-326).  A [m][n], B [m], X0 [n][r] (columns).  Returns a dict."""
    rt, ct = np.dtype(dtype).type, ctype(dtype)
    A = np.asarray(A, ct)
    B = np.asarray(B, rt)
    X = np.asarray(X0, ct).reshape(A.shape[1], -1).copy()
    m, n = A.shape
    r = X.shape[1]
    if U is None:
        U = pinv(A, dtype)
    U = np.asarray(U, ct)
    tol_rel, tol_abs, rho = rt(tol_rel), rt(tol_abs), rt(rho)
    AX = A @ X
    if scale_by_row:
        X = X * (_norm(B) / _norm(AX))
    else:
        X = X * (_norm(B) / np.sqrt(np.sum(np.abs(AX) ** 2, axis=0)))[None, :]
    AX = A @ X
    Y = normalize_rows(AX, B, scale_by_row)
    AtY = A.conj().T @ Y
    M = np.zeros((m, r), ct)
    mu = rt(mu0)
    opt_obj, last_res = rt(np.inf), rt(np.inf)
    opt_X = opt_Y = None
    objcol, converged, it = 0, False, 0
    mus = []
    for it in range(1, maxiter + 1):
        Y0, AtY0 = Y, AtY
        X = U @ (Y - M / mu)
        AX = A @ X
        Y = argmin_y(AX, B, M, mu, scale_by_row)
        AtY = A.conj().T @ Y
        J = AX - Y
        M = M + mu * J
        if scale_by_row:
            obj, j = _norm(np.sqrt(np.sum(np.abs(AX) ** 2, axis=1)) - B), 0
        else:
            obj, j = _first_min_skipping_nan(np.sqrt(np.sum((np.abs(AX) - B[:, None]) ** 2, axis=0)))
        if obj < opt_obj:
            opt_obj, objcol, opt_X, opt_Y = obj, j, X.copy(), Y.copy()
        res_prim = _norm(J)
        res_dual = mu * _norm(AtY - AtY0)
        res_comb = np.sqrt(res_prim ** 2 + _norm(Y - Y0) ** 2)
        mx = max(_norm(AX), _norm(Y))
        th_prim = tol_abs * np.sqrt(rt(m * r)) + tol_rel * mx
        th_dual = tol_abs * np.sqrt(rt(n * r)) + tol_rel * _norm(AtY)
        th_comb = tol_abs * np.sqrt(rt(m * r * 2)) + tol_rel * np.sqrt(mx ** 2 + _norm(Y) ** 2)
        mus.append(mu)
        if (res_prim < th_prim and res_dual < th_dual) or res_comb < th_comb:
            converged = True
            break
        if res_comb > last_res * rt(0.9):
            mu = mu * rho
        last_res = res_comb
    if opt_X is None:   # the reference would raise (opt_X undefined); the kernel returns the last iterate
        opt_X, opt_Y = X, Y
    if scale_by_row:
        Xr, Yr = opt_X, opt_Y
    else:
        Xr, Yr = opt_X[:, objcol], opt_Y[:, objcol]
    return dict(X=Xr, Y=Yr, Xall=opt_X, Yall=opt_Y, iters=it, objcol=objcol, opt_obj=opt_obj, mu=mu,
                mus=np.array(mus, rt), converged=converged)


def r_rule(s2, r, m, n):
    """:187-190 (and its copy :203-206): the column count from the descending spectrum."""
    if s2[:r].sum() >= s2.sum() * 0.9:
        r = max(int(np.flatnonzero(np.cumsum(s2) >= s2.sum() * 0.9)[0]) + 1, 3)
        r = min(r, m, n)
    return r


def spectral_columns(A, B, r):
    """X = V(:, 1:r) diag(sqrt(s2(1:r))) of :176-191 without the column-count rule (r <= min(m, n))."""
    return _spectrum(A, B)[0][:, :r]


def _spectrum(A, B):
    A = np.asarray(A, np.complex128)
    B = np.asarray(B, np.float64)
    an = np.sqrt(np.sum(np.abs(A) ** 2, axis=1))
    sc = np.where(an != 0, B / np.where(an != 0, an, 1), 1.0)
    As = A * sc[:, None]
    AtA = As.conj().T @ As
    AtA = (AtA + AtA.conj().T) / 2   # MATLAB's eig takes the Hermitian path for As' * As
    lam, V = np.linalg.eigh(AtA)
    s2 = np.maximum(0, lam)
    idx = np.argsort(-s2, kind="stable")
    s2 = s2[idx]
    return V[:, idx] * np.sqrt(s2)[None, :], s2


def spectral_init(A, B, r):
    """:176-207, float64.  Returns X [n][r_used] and (r after the first block, r after its copy)."""
    m, n = np.shape(A)
    Xf, s2 = _spectrum(A, B)
    r1 = r_rule(s2, r, m, n)
    r2 = r_rule(s2, r1, m, n)
    return Xf[:, :r2], (r1, r2)


def infer_min_l2_impl(A, B, r, dtype=np.float64, maxiter=500, tol_rel=1e-4, tol_abs=1e-8):
    """inferMinL2Impl (:67-227).  Returns X [n], Y [m] and a dict of the stages."""
    U = pinv(A, dtype)
    X0, (r1, r2) = spectral_init(A, B, r)
    s1 = infer_admm(A, B, X0, True, dtype, maxiter, tol_rel, tol_abs, U)
    Xs = np.asarray(s1["X"], np.complex128)
    G = Xs.conj().T @ Xs
    _, Vx = np.linalg.eigh((G + G.conj().T) / 2)
    Xrot = np.asarray(s1["X"], ctype(dtype)) @ Vx.astype(ctype(dtype))
    s2 = infer_admm(A, B, Xrot, False, dtype, maxiter, tol_rel, tol_abs, U)
    return s2["X"], s2["Y"], dict(r=(r1, r2), X0=X0, stage1=s1, Xrot=Xrot, stage2=s2)


def infer_min_l2(A, B, train_idx, dtype=np.float64, r=20, maxiter=500, tol_rel=1e-4, tol_abs=1e-8):
    """inferMinL2 (:1-65) with the partition given.  Returns X [n], Y, quality and a dict (stage iters, r, status)."""
    rt, ct = np.dtype(dtype).type, ctype(dtype)
    A = np.asarray(A, ct)
    B = np.asarray(B, rt)
    m, n = A.shape
    r = min(r, m, n)
    a_norm = _norm(A) / np.sqrt(rt(m))
    if a_norm < tol_abs:
        a_norm = rt(1)
    b_norm = _norm(B)
    if b_norm < tol_abs:
        b_norm = rt(1)
    A = A / a_norm
    B = B / b_norm
    train_idx = np.asarray(train_idx, np.int64)
    test_idx = np.setdiff1d(np.arange(m), train_idx)
    X, Y, info = infer_min_l2_impl(A[train_idx], B[train_idx], r, dtype, maxiter, tol_rel, tol_abs)
    with np.errstate(invalid="ignore", divide="ignore"):
        quality = 1 - _norm(np.abs(A[test_idx] @ X) - B[test_idx]) / _norm(B[test_idx])
    iters = [info["stage1"]["iters"], info["stage2"]["iters"], 0]
    rolled = False
    if quality > 0.6:
        X0, Y0 = X, Y
        s3 = infer_admm(A, B, X0[:, None], True, dtype, maxiter, tol_rel, tol_abs)
        X, Y = s3["X"][:, 0], s3["Y"][:, 0]
        iters[2] = s3["iters"]
        info["stage3"] = s3
        if np.abs(np.vdot(X0, X)) / _norm(X0) / _norm(X) < 0.6:
            X, Y, rolled = X0, Y0, True
    info.update(stage_iters=iters, rolled_back=rolled, r_used=info["r"][1])
    return X * (b_norm / a_norm), Y * (b_norm / a_norm), quality, info


# ---------------------------------------------------------------- the cases the CPU and the GPU tests share
import concurrent.futures  # noqa: E402
import functools  # noqa: E402

U64 = 2.0 ** -53
SHAPES = ((5, 17), (16, 48), (33, 130), (64, 256), (20, 17))   # (n, m); the last one is m <= n
NB = 8
# mode -> (scale_by_row, columns (None: min(20, n)), maxiter)
MODES = {"row": (True, None, 500), "col40": (False, None, 40), "r1_40": (True, 1, 40), "col": (False, None, 500),
         "r1": (True, 1, 500)}


@functools.lru_cache(maxsize=None)
def problem(n, m, nb=NB, seed=20, snr_db=30.0):
    """A phase-code A / sqrt(n), Gaussian channels, magnitudes at ``snr_db`` and a Gaussian X0 [nb][min(20, n)][n]."""
    rng = np.random.default_rng([seed, n, m])
    A = np.exp(0.5j * np.pi * rng.integers(0, 4, (m, n))) / np.sqrt(n)
    x = rng.standard_normal((nb, n)) + 1j * rng.standard_normal((nb, n))
    y = x @ A.T
    sig = np.sqrt(np.mean(np.abs(y) ** 2) / 10 ** (snr_db / 10) / 2)
    B = np.abs(y + sig * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape)))
    r = min(20, n)
    X0 = rng.standard_normal((nb, r, n)) + 1j * rng.standard_normal((nb, r, n))
    if m > n:   # the r leading columns of the spectral initialisation (no column-count rule); m <= n keeps the Gaussian
        X0 = np.stack([spectral_columns(A, B[b], r).T for b in range(nb)])
    return A, B, X0, x


def mu_steps(o, mu0=1e-3, rho=1.03):
    """The mu schedule as integers: how often mu had been raised before each iteration."""
    return np.rint(np.log(np.asarray(o["mus"], np.float64) / mu0) / np.log(rho)).astype(np.int64)


def same_decisions(a, b):
    return a["iters"] == b["iters"] and a["objcol"] == b["objcol"] and a["converged"] == b["converged"] \
        and np.array_equal(mu_steps(a), mu_steps(b))


def _dist(a, b):
    return float(np.sqrt(np.sum(np.abs(np.asarray(a, np.clongdouble) - np.asarray(b, np.clongdouble)) ** 2)))


@functools.lru_cache(maxsize=None)
def stage_case(n, m, mode):
    """The oracle's runs of one shape and mode: per realisation the long-double run (the target), the float64 run and
    the float64 run on permuted rows, whether the three agree in every decision (the case "counts"), and the spread
    of Xall, Yall (all columns), X, Y (what the stage returns) and opt_obj: the larger distance of the two float64 runs from the target."""
    sbr, cols, maxiter = MODES[mode]
    A, B, X0, _ = problem(n, m)
    X0 = X0 if cols is None else X0[:, :cols]
    perm = np.random.default_rng([n, m, 1]).permutation(m)
    def one(b):
        o_ld = infer_admm(A, B[b], X0[b].T, sbr, np.longdouble, maxiter)
        o_64 = infer_admm(A, B[b], X0[b].T, sbr, np.float64, maxiter)
        o_pm = infer_admm(A[perm], B[b][perm], X0[b].T, sbr, np.float64, maxiter)
        for k in ("Yall", "Y"):   # back to A's row order
            Yp = np.empty_like(o_pm[k])
            Yp[perm] = o_pm[k]
            o_pm[k] = Yp
        # X and Y are what the stage returns: all columns in the row form, the best column in the per-column form
        # (the same column in the three runs of a counting case)
        sp = {k: max(_dist(o_64[k], o_ld[k]), _dist(o_pm[k], o_ld[k])) for k in ("Xall", "Yall", "X", "Y", "opt_obj")}
        return o_ld, o_64, o_pm, same_decisions(o_ld, o_64) and same_decisions(o_ld, o_pm), sp

    # (the realisations side by side: numpy's long-double products run outside the interpreter lock)
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(B)) as ex:
        runs = list(ex.map(one, range(len(B))))
    ref, f64, prm, counts, spread = (list(v) for v in zip(*runs))
    return dict(A=A, B=B, X0=X0, scale_by_row=sbr, maxiter=maxiter, ref=ref, f64=f64, perm=prm, counts=counts,
                spread=spread)


def bound(n, m, ref_value, spread):
    """max((m + n) u ||ref||, 16 x spread): the classical bound of sums of that length, or the recursion's own
    float64 spread at this realisation where that is larger (16 covers the device's summation order)."""
    nr = float(np.sqrt(np.sum(np.abs(np.asarray(ref_value, np.clongdouble)) ** 2)))
    return max((m + n) * U64 * nr, 16 * spread)
