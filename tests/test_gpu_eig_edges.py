"""The Hermitian eigensolver chain (Householder reduction, trieig_kernel, back-transform; csrc/ace_spectral.hip and
csrc/ace_heev2.hip) on the inputs where bisection plus inverse iteration classically fail: exact and near
multiplicities, low rank, graded spectra, matrices whose tridiagonal splits exactly, and the orders on either side of
every switch between two kernels.  The matrices, their decomposition known by construction, the checker and the
tolerances are tests/eig_ref.py's (self-tested on the CPU by tests/test_eig_ref.py); nothing here is compared with
an f64 eigh.  SpectralInitialize is run on inputs whose X X^H is known in closed form (mutually orthogonal rows) and
against oracle/ace_oracle.py::spectral_initialize where the rank falls below r.

Every check prints its worst error / bound (pytest -s shows them; DESIGN.md section 4 tabulates them).  The exactly
diagonal matrix with a 16-fold entry (diag_mult_16, d = 256) is the case that found the inverse-iteration fallback's
rank-three start vectors: before the fix its shrunk matrix was at 2.9 times the bound."""
import numpy as np
import pytest

import ace_oracle as O
import eig_ref as R

pytestmark = pytest.mark.gpu

SMALL = (2, 3, 5, 31, 32, 33, 95, 96, 97, 129)


def _worse(a, b):
    return {k: max(a.get(k, 0.0), b[k]) for k in b}


def _expect_side(c):
    """path + 4 returns the eigenpairs at or below tau when more than half lie above it, unless those at or below
    come in a cluster of more than 8 (trieig_kernel's TE_SIDE_CL)."""
    above = int(np.sum(c.w > c.tau))
    big = max(len(g.idx) for g in c.groups if c.w[g.idx[0]] <= c.tau)
    return 2 * above > c.d and big <= 8


def _run_case(c, path, label):
    from ace_amd import prox_eig_host
    d, above = c.d, int(np.sum(c.w > c.tau))
    taus = [c.tau] + ([c.below] if c.full_ok else [])
    lam, V, k = prox_eig_host(np.stack([c.A] * len(taus)), np.array(taus), path=path)
    worst = {}
    assert k[0] == above, (label, path, k[0], above)
    worst = _worse(worst, R.check_case(c, lam[0], V[0], k[0], c.tau))
    if c.full_ok:     # tau below the spectrum: the whole decomposition
        assert k[1] == d, (label, path, k[1])
        worst = _worse(worst, R.check_case(c, lam[1], V[1], k[1], c.below))
    ls, Vs, ks = prox_eig_host(c.A[None], np.array([c.tau]), path=path + 4)
    assert ks[0] == (above - d if _expect_side(c) else above), (label, path + 4, ks[0], above)
    worst = _worse(worst, R.check_case(c, ls[0], Vs[0], ks[0], c.tau))
    print(f"EIGEDGE {label} d={d} path={path} " + " ".join(f"{n}={v:.3g}" for n, v in worst.items()))
    return worst


@pytest.mark.parametrize("d", R.DIMS)
@pytest.mark.parametrize("name", R.CASES)
def test_families(gpu, name, d):
    """Every family through the unblocked, blocked and two-stage reductions: the pairs above tau, the smaller side of
    tau (path + 4) and, where no cluster exceeds 16, the whole decomposition."""
    c = R.case(name, d)
    for path in (0, 1, 2):
        _run_case(c, path, name)


def test_side_outcomes(gpu):
    """Six zeros below tau: the zero cluster is the smaller side, k = -6.  24 zeros and 40 distinct values above tau at
    d = 64: the cluster is larger than TE_SIDE_CL, so the solver flips back and returns k = +40."""
    from ace_amd import prox_eig_host
    for path in (0, 1, 2):
        for name, want in (("lowrank_6", -6), ("lowrank_flip", 40)):
            c = R.case(name, 64)
            lam, V, k = prox_eig_host(c.A[None], np.array([c.tau]), path=path + 4)
            assert k[0] == want, (name, path, k[0])
            R.check_case(c, lam[0], V[0], k[0], c.tau)


def _small_cases(d):
    return [R.random_hermitian(d, 0)] + ([R.small_mult(d)] if d >= 3 else [])


@pytest.mark.parametrize("d", SMALL)
def test_small_and_switch_orders(gpu, d):
    """Orders around wy_path's d >= 96 and heev2_eligible's d >= 32, and the smallest the entry accepts, through the
    one-stage paths; below 32 path 2 is path 1."""
    from ace_amd import prox_eig_host
    for c in _small_cases(d):
        res = {}
        for path in (0, 1):
            worst = {}
            for tau in (c.tau, c.below):
                lam, V, k = prox_eig_host(c.A[None], np.array([tau]), path=path)
                worst = _worse(worst, R.check_case(c, lam[0], V[0], k[0], tau))
                res[path, tau] = (lam, V, k)
            print(f"EIGEDGE small:{c.name} d={d} path={path} " + " ".join(f"{n}={v:.3g}" for n, v in worst.items()))
        if d == 31:
            for tau in (c.tau, c.below):
                (l2, V2, k2), (l1, V1, k1) = prox_eig_host(c.A[None], np.array([tau]), path=2), res[1, tau]
                kc = int(k1[0])      # (rows past k are not written)
                assert k2[0] == kc and np.array_equal(l2[0, :kc], l1[0, :kc]) and np.array_equal(V2[0, :kc], V1[0, :kc])


@pytest.mark.parametrize("path", [0, 1, 2, 5, 6])
def test_batch_position_on_cluster_paths(gpu, path):
    """A clustered matrix next to a random one: each result is bit for bit the one of the matrix run alone."""
    from ace_amd import prox_eig_host
    cs = [R.case("mult_16", 256), R.random_hermitian(256, 1), R.case("tight6_1e-11", 256), R.case("lowrank_6", 256)]
    A, tau = np.stack([c.A for c in cs]), np.array([c.tau for c in cs])
    lam, V, k = prox_eig_host(A, tau, path=path)
    for b in range(len(cs)):
        l1, V1, k1 = prox_eig_host(A[b:b + 1], tau[b:b + 1], path=path)
        kc = abs(int(k[b]))
        assert k1[0] == k[b] and np.array_equal(l1[0, :kc], lam[b, :kc]) and np.array_equal(V1[0, :kc], V[b, :kc]), b


# ---------------------------------------------------------------- SpectralInitialize
def _no_noconv(st):
    from ace_amd import ACE_ST_EIG_NOCONV
    assert not np.any(np.asarray(st) & ACE_ST_EIG_NOCONV), st


def _orth_rows(rng, m, n):
    """A with mutually orthogonal rows a_i = c_i e_col(i): the first n rows hit distinct columns, later ones repeat."""
    perm = rng.permutation(n)
    col = perm[np.arange(m) % n]
    c = rng.uniform(0.5, 2.0, m) * np.exp(2j * np.pi * rng.uniform(size=m))
    A = np.zeros((m, n), np.complex128)
    A[np.arange(m), col] = c
    return A, col


# eigenvalues of As^H As wanted in the top r = 12: 5 equal, 2 equal, 5 distinct; then a gap of 0.02 (relative)
_TOP = np.array([4.0, 3.5] + [3.0] * 5 + [2.5, 2.2] + [2.0] * 2 + [1.8]) ** 2
_REST = 1.7 ** 2


@pytest.mark.parametrize("m,n", [(40, 64), (64, 64), (100, 64), (90, 49)])
def test_spectral_initialize_orthogonal_rows(gpu, m, n):
    """As^H As = sum_i B_i^2 e_col(i) e_col(i)^T is diagonal (K = A A^H as well where m <= n: the tridiagonal splits
    everywhere), so X X^H over the top r is a known diagonal matrix; through the dual (m <= n) and the primal
    (m > n, repeated basis rows) path."""
    from ace_amd import SpectralInitialize
    rng = np.random.default_rng(1000 * m + n)
    r = 12
    A, col = _orth_rows(rng, m, n)
    nd = min(m, n)                              # distinct columns hit
    s = np.concatenate([_TOP, _REST * rng.uniform(0.0, 1.0, nd - r)])[rng.permutation(nd)]    # per column hit
    s[rng.choice(np.flatnonzero(s < _REST), 3, replace=False)] = 0.0      # and a few zero magnitudes
    B = np.zeros((2, m))
    B[0, :nd] = np.sqrt(s)                      # (repeated rows weighted zero)
    B[1, :nd] = (0.5 if m <= n else 1.0) * B[0, :nd]
    assert m < 2 * n
    for i in range(n, m):                       # a repeated row takes a share of its column's eigenvalue
        f = rng.uniform(0.2, 0.8)
        B[1, i], B[1, i - n] = np.sqrt(s[i - n] * f), np.sqrt(s[i - n] * (1 - f))
    X, st = SpectralInitialize(A, B, r, return_status=True)
    _no_noconv(st)
    for b in range(2):
        ev = np.zeros(n)
        np.add.at(ev, col, B[b] ** 2)           # the eigenvalue of e_j
        top = np.sort(ev)[::-1]
        assert (top[r - 1] - top[r]) / top[0] >= 1e-3
        P = np.diag(np.where(ev >= top[r - 1], ev, 0.0))
        assert np.isfinite(X[b]).all()
        e = np.linalg.norm(X[b] @ X[b].conj().T - P) / np.linalg.norm(P)
        print(f"EIGEDGE spectral:orth m={m} n={n} b={b} err/bound={e / 1e-10:.3g}")
        assert e <= 1e-10, (b, e)


@pytest.mark.parametrize("tx,m,r,nnz", [(8, 17, 12, 9), (16, 40, 20, 12)])
def test_spectral_initialize_rank_below_r(gpu, tx, m, r, nnz):
    """All but nnz < r magnitudes zero (the first and the last row among them): the zero eigenvalue's cluster lies
    inside the top r."""
    from ace_amd import SpectralInitialize, synth
    A, B, _, _ = synth.problem(20 + tx, 0, 3, m, tx, tx)
    A, B = A[0], B.copy()
    rng = np.random.default_rng(m)
    for b in range(B.shape[0]):
        keep = rng.choice(np.arange(1, m - 1), nnz, replace=False)
        z = np.ones(m, bool)
        z[keep] = False
        B[b, z] = 0.0
    X, st = SpectralInitialize(A, B, r, return_status=True)
    _no_noconv(st)
    for b in range(B.shape[0]):
        Xo = O.spectral_initialize(A, B[b], r)
        As = A * (B[b] / np.linalg.norm(A, axis=1))[:, None]
        nc = np.linalg.norm(As.conj().T @ As)
        assert np.isfinite(X[b]).all()
        tail = np.linalg.norm(X[b][:, nnz:], axis=0).max()
        P, Po = X[b] @ X[b].conj().T, Xo @ Xo.conj().T
        e = np.linalg.norm(P - Po) / np.linalg.norm(Po)
        bound = np.sqrt(1e-11 * nc)
        print(f"EIGEDGE spectral:rank m={m} b={b} err/bound={e / 1e-10:.3g} tail/bound={tail / bound:.3g}")
        assert tail <= bound, (b, tail)
        assert e <= 1e-10, (b, e)


def test_spectral_initialize_repeated_row(gpu):
    """A repeated row of A: K = A A^H is singular."""
    from ace_amd import SpectralInitialize, synth
    A, B, _, _ = synth.problem(31, 0, 2, 40, 8, 8)
    A = A[0].copy()
    A[5] = A[2]
    X, st = SpectralInitialize(A, B, 12, return_status=True)
    _no_noconv(st)
    for b in range(B.shape[0]):
        Xo = O.spectral_initialize(A, B[b], 12)
        P, Po = X[b] @ X[b].conj().T, Xo @ Xo.conj().T
        e = np.linalg.norm(P - Po) / np.linalg.norm(Po)
        print(f"EIGEDGE spectral:reprow b={b} err/bound={e / 1e-10:.3g}")
        assert np.isfinite(X[b]).all() and e <= 1e-10, (b, e)
