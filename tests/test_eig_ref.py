"""CPU self-test of tests/eig_ref.py: the constructions are what they claim, numpy's eigh passes the checker on every
case and order the GPU tests use with a 10x margin, and the checker fails on each planted error."""
import numpy as np
import pytest

import eig_ref as R

LD = np.longdouble
SMALL = (2, 3, 5, 31, 32, 33, 95, 96, 97, 129)     # the orders of test_gpu_eig_edges.py's small-order test


def _eigh(A, tau, side=False):
    """numpy's eigh in the layout of ace_amd.prox_eig_host."""
    w, U = np.linalg.eigh(A)
    d = len(w)
    if side:
        kc = int(np.sum(w <= tau))
        lam, V, k = w.copy(), U.T.copy(), -kc
    else:
        lam, V, k = w[::-1].copy(), U[:, ::-1].T.copy(), int(np.sum(w > tau))
    lam[abs(k):] = 0.0
    V[abs(k):] = 0.0
    return lam, V, k


def test_unitary_and_jacobi_are_long_double_accurate():
    Q = R.unitary(64, 0)
    assert np.abs(Q.conj().T @ Q - np.eye(64)).max() <= 1e-17
    T, w, U = R._wilkinson_block(21, True)
    T = T.astype(LD)
    assert np.abs(U.T @ U - np.eye(42)).max() <= 1e-17
    assert np.abs(T @ U - U * w[None, :]).max() <= 1e-17 * 11
    # W21+'s largest pair: 10.746194182903..., agreeing to ~1e-14
    top = np.sort(R._wilkinson_block(21, False)[1])[-2:]
    assert abs(float(top[1]) - 10.746194182903393) <= 1e-13 and 0 < float(top[1] - top[0]) < 1e-12


@pytest.mark.parametrize("d", R.DIMS)
def test_cases_are_what_they_claim(d):
    sizes = lambda c: sorted((len(g.idx) for g in c.groups if len(g.idx) > 1), reverse=True)
    for name in R.CASES:
        c = R.case(name, d)
        assert c.A.shape == (d, d) and np.array_equal(c.A, c.A.conj().T), name
        assert np.all(np.diff(c.w) <= 0) and sum(len(g.idx) for g in c.groups) == d, name
        n2 = np.abs(c.w).max()
        # every group >= SEP ||A||_2 from the rest, tau mid-gap between two groups
        assert all(g.gap >= R.SEP * n2 * (1 - 1e-12) for g in c.groups), name
        above = int(np.sum(c.w > c.tau))
        assert any(g.idx[0] == above for g in c.groups), name
        assert min(c.w[above - 1] - c.tau, c.tau - c.w[above]) >= 0.49 * R.SEP * n2, name
        if c.full_ok:
            assert max(len(g.idx) for g in c.groups) <= 16, name
    assert sizes(R.case("mult_33322", d)) == [3, 3, 3, 2, 2]
    assert sizes(R.case("mult_6", d)) == [6] and sizes(R.case("mult_16", d)) == [16]
    assert sizes(R.case("tight4_1e-7", d)) == [4]
    assert sizes(R.case("tight6_1e-11", d)) == [6] == sizes(R.case("tight6_1e-7", d))
    assert sizes(R.case("ortol_pairs", d)) == [2, 2]
    assert sizes(R.case("lowrank_6", d)) == [6] and sizes(R.case("lowrank_flip", d)) == [(3 * d) // 8]
    assert sizes(R.case("block_diag", d)) == [3, 2]
    c = R.case("lowrank_flip", d)      # more than half above tau, the rest one cluster of more than 8
    assert 2 * int(np.sum(c.w > c.tau)) > d and d - int(np.sum(c.w > c.tau)) > 8
    for name, want in (("diag_repeated", [3, 3, 3, 2, 2]), ("diag_mult_16", [16])):
        c = R.case(name, d)
        assert np.count_nonzero(c.A - np.diag(np.diag(c.A))) == 0 and sizes(c) == want
    for name, s in (("mult_33322_up", 2.0 ** 100), ("mult_33322_down", 2.0 ** -100)):
        assert np.array_equal(R.case(name, d).A, R.case("mult_33322", d).A * s)
    for name in ("wilkinson", "wilkinson_glued"):    # real tridiagonal block, then exact zeros in e
        A = R.case(name, d).A
        assert np.count_nonzero(np.triu(A, 2)) == 0 and np.count_nonzero(np.diag(A, 1)) in (20, 41, 29)


@pytest.mark.parametrize("d", R.DIMS)
@pytest.mark.parametrize("name", R.CASES)
def test_eigh_passes_with_margin(name, d):
    c = R.case(name, d)
    runs = [(c.tau, False), (c.tau, True)] + ([(c.below, False)] if c.full_ok else [])
    for tau, side in runs:
        lam, V, k = _eigh(c.A, tau, side)
        R.check_case(c, lam, V, k, tau, margin=0.1)


@pytest.mark.parametrize("d", SMALL)
def test_eigh_passes_small_orders(d):
    cs = [R.random_hermitian(d, 0)] + ([R.small_mult(d)] if d >= 3 else [])
    for c in cs:
        for tau in (c.tau, c.below):
            lam, V, k = _eigh(c.A, tau)
            R.check_case(c, lam, V, k, tau, margin=0.1)


# ---------------------------------------------------------------- planted errors
@pytest.fixture(scope="module")
def good():
    c = R.case("mult_33322", 64)
    lam, V, k = _eigh(c.A, c.tau)
    R.check_case(c, lam, V, k, c.tau)
    return c, lam, V, k


def _fails(c, lam, V, k, which):
    with pytest.raises(R.EigCheckError) as e:
        R.check_case(c, lam, V, k, c.tau)
    assert e.value.which in which, e.value


def test_catches_duplicated_cluster_vector(good):
    c, lam, V, k = good
    V = V.copy()
    V[1] = V[0]                      # rows 0..2 are the triple eigenvalue's vectors
    V[1] /= np.linalg.norm(V[1])
    _fails(c, lam, V, k, ("orth",))
    # and where only the subspace shows it: the duplicate replaced by a unit vector orthogonal to the kept ones
    # but outside the cluster's subspace
    x = c.groups[-1].basis[:, 0].copy()
    V[1] = x / np.linalg.norm(x)
    _fails(c, lam, V, k, ("res", "proj", "shrunk", "orth"))


def test_catches_rotation_out_of_cluster(good):
    """Vector 0 (triple eigenvalue 1.0) and vector 3 (the next group, 0.07 away) rotated into each other by 1e-7:
    still orthonormal, the residual moves by 1e-7 * 0.07 = 7e-9 ||A||_2 and both subspaces by 1e-7."""
    c, lam, V, k = good
    V = V.copy()
    t = 1e-7
    V[0], V[3] = np.cos(t) * V[0] + np.sin(t) * V[3], np.cos(t) * V[3] - np.sin(t) * V[0]
    assert np.abs(V[:k].conj() @ V[:k].T - np.eye(k)).max() <= 1e-14
    _fails(c, lam, V, k, ("res",))


def test_catches_swapped_eigenvalues(good):
    c, lam, V, k = good
    lam = lam.copy()
    lam[2], lam[3] = lam[3], lam[2]
    _fails(c, lam, V, k, ("eig",))


def test_catches_scaled_vector(good):
    c, lam, V, k = good
    V = V.copy()
    V[5] *= 1 + 1e-9
    _fails(c, lam, V, k, ("orth",))


def test_catches_count_off_by_one(good):
    c, lam, V, k = good
    _fails(c, lam, V, k - 1, ("count",))
    _fails(c, lam, V, k + 1, ("count",))
    _fails(c, lam, V, -k, ("count",))
