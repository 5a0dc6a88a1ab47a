"""Hermitian matrices whose eigen-decomposition is known by construction, and one checker for what an
eigensolver returns on them (tests/test_gpu_eig_edges.py; self-tested on the CPU by tests/test_eig_ref.py).

(a) Construction
----------------
``unitary(d, seed)`` is a product of d random Householder reflectors in ``np.clongdouble`` (unitary to ~1e-18).
A case is A = Q diag(w) Q^H formed in long double, hermitised and rounded to complex128: its eigenvalues are w and
the invariant subspace of any set of eigenvalues is the matching set of columns of Q, both known far better than
an f64 ``eigh`` gives them (the rounding moves them by 2^-53 ||A||, which is what any f64 solver is given).
The cases of family 5 are taken without Q: an exactly diagonal matrix (Q is a permutation), block-diagonal
matrices (Q is block diagonal) and Wilkinson's W21+, alone and as two glued copies, next to a diagonal block;
the Wilkinson blocks' decomposition comes from a cyclic Jacobi iteration in long double (``jacobi_ld``).

(b) Families (``CASES``; every one exists at every d in ``DIMS``, ``case(name, d)``)
-----------------------------------------------------------------------------------
1  exact multiplicities above tau: (3, 3, 3, 2, 2, distinct ...), one of 6, one of 16;
2  tight but not equal: four and six eigenvalues 1e-7 ||A|| apart, six 1e-11 ||A|| apart, pairs 3e-6 and 3e-5 apart;
3  low-rank PSD, tau between the zeros and the rest: 6 zeros, and 3 d / 8 zeros (24 at d = 64);
4  graded, 2^(-40 j / d);
5  exactly diagonal with repeated entries ((3, 3, 3, 2, 2), and one entry 16 times), block diagonal with eigenvalues
   shared between blocks, Wilkinson, glued Wilkinson;
6  family 1's first case times 2^100 and 2^-100.  (A reduction's reflector norm is an unscaled square root of a sum
   of squares, so powers beyond ~2^500 would test overflow of that sum; that is not the aim here.)
Multiplicities stay <= 16 among the vectors a test asks for (the solvers under test orthogonalise a cluster
serially): ``full_ok`` is False where the whole decomposition would hold a larger cluster.

(c) Groups
----------
The sorted spectrum is cut wherever two neighbours are at least SEP ||A||_2 apart (SEP = 1e-4); the runs in between
are the groups (a multiple eigenvalue, a tight cluster, or a single well-separated eigenvalue) and ``gap`` is a
group's distance from the rest of the spectrum.  Only the group's subspace is determined; the vectors inside it
are not.  Every tau lies mid-gap between two groups.

(d) Checker and tolerances
--------------------------
``check`` asserts only quantities that do not depend on a vector's phase or on a rotation inside a group: the kept
count; the eigenvalues; the residual max_q ||A v_q - lam_q v_q||; orthonormality max |V^H V - I|; the shrunk
matrix sum (lam - tau) v v^H against the constructed one; and per group the distance of span(V_g) from
span(Q_g), max(||(I - Q_g Q_g^H) V_g||_2, ||(I - V_g V_g^H) Q_g||_2), which for orthonormal bases of equal
dimension is ||V_g V_g^H - Q_g Q_g^H||_2 (the sine of the largest principal angle).  The tolerances are the
project's, not measured on the code under test: TOL = 1e-11 ||A||_F for eigenvalues, residual and shrunk matrix and
ORTH = 1e-10 for orthonormality are the figures tests/test_gpu_heev2.py already uses; a solver with backward
error E, ||E||_F <= 1e-11 ||A||_F, moves a group's subspace by at most ||E||_F / gap (Davis-Kahan), so a group's
bound is 1e-11 ||A||_F / gap.  ``margin`` scales every bound (the CPU self-test asks numpy's eigh for 10x).
"""
import dataclasses
import functools

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
DIMS = (33, 64, 100, 256)
SEP = 1e-4
TOL = 1e-11
ORTH = 1e-10


class EigCheckError(AssertionError):
    """which: the first failed check (count, eig, orth, res, shrunk, proj)."""

    def __init__(self, which, msg):
        super().__init__(f"{which}: {msg}")
        self.which = which


@dataclasses.dataclass(frozen=True)
class Group:
    idx: np.ndarray      # positions in the descending spectrum
    basis: np.ndarray    # [d, len(idx)] complex128, orthonormal columns
    gap: float           # distance of the group's eigenvalues from the rest of the spectrum


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    A: np.ndarray        # [d, d] complex128, exactly Hermitian
    w: np.ndarray        # [d] float64, descending (the constructed eigenvalues, rounded)
    groups: tuple
    tau: float           # mid-gap between two groups
    full_ok: bool        # the whole decomposition holds no cluster of more than 16

    @property
    def d(self):
        return self.A.shape[0]

    @property
    def below(self):     # a threshold below the whole spectrum: every pair is kept
        return float(self.w[-1] - 0.25 * np.abs(self.w).max())


# ---------------------------------------------------------------- long-double building blocks
def _crandn(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(CLD)


@functools.lru_cache(maxsize=None)
def unitary(d, seed):
    """Product of d random Householder reflectors, clongdouble."""
    rng = np.random.default_rng([d, seed])
    Q = np.eye(d, dtype=CLD)
    for _ in range(d):
        v = _crandn(rng, d)
        v /= np.sqrt(np.sum(v.real * v.real + v.imag * v.imag))
        Q -= np.outer(2 * (Q @ v), v.conj())
    Q.setflags(write=False)
    return Q


def jacobi_ld(T):
    """Eigen-decomposition of a small real symmetric matrix by cyclic Jacobi in long double: (w, U), T U = U diag(w)."""
    A = np.array(T, dtype=LD)
    n = A.shape[0]
    U = np.eye(n, dtype=LD)
    scale = np.sqrt(np.sum(A * A))
    for _ in range(40):
        off = np.sqrt(np.sum(np.triu(A, 1) ** 2) * 2)
        if not off > 1e-20 * scale:
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                if A[p, q] == 0:
                    continue
                th = (A[q, q] - A[p, p]) / (2 * A[p, q])
                t = (1 if th >= 0 else -1) / (abs(th) + np.sqrt(th * th + 1))
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                for M in (A, U):
                    mp, mq = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * mp - s * mq, s * mp + c * mq
                rp, rq = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * rp - s * rq, s * rp + c * rq
                A[p, q] = A[q, p] = 0
    return np.diag(A).copy(), U


def wilkinson(n):
    """Wilkinson's W_n^+ (n odd): diagonal |i - (n-1)/2|, off-diagonals 1."""
    m = (n - 1) // 2
    return np.diag(np.abs(np.arange(n) - m).astype(float)) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)


def _fill(rng, n, lo, hi):
    """n values in [lo, hi], neighbours at least half the even spacing apart."""
    if n <= 0:
        return np.zeros(0)
    h = (hi - lo) / n
    return lo + h * (np.arange(n) + 0.5 + 0.25 * rng.uniform(-1, 1, n))


# ---------------------------------------------------------------- spectra (||A||_2 = 1 before scaling)
def _spec_mult(rng, d, mult):
    top = np.concatenate([np.full(m, 1.0 - 0.07 * i) for i, m in enumerate(mult)])
    return np.concatenate([top, _fill(rng, d - len(top), -0.9, 0.6)])


def _spectrum(name, d, rng):
    """(w, number kept by tau, full_ok)."""
    if name in ("mult_33322", "mult_33322_up", "mult_33322_down", "diag_repeated"):
        w = _spec_mult(rng, d, (3, 3, 3, 2, 2))
        return w, 13 + (d - 13) // 2 + 2, True        # more than half above tau: path + 4 returns the lower side
    if name == "mult_6":
        return _spec_mult(rng, d, (1, 6, 1)), 8 + (d - 8) // 3, True
    if name in ("mult_16", "diag_mult_16"):
        return _spec_mult(rng, d, (1, 16)), 17 + (d - 17) // 4, True
    if name == "tight4_1e-7":
        w = np.concatenate([[1.0], 0.9 + 1e-7 * np.arange(4), _fill(rng, d - 5, -0.9, 0.6)])
        return w, 5 + (d - 5) // 3, True
    if name in ("tight6_1e-11", "tight6_1e-7"):
        w = np.concatenate([[1.0], 0.9 + float(name[7:]) * np.arange(6), _fill(rng, d - 7, -0.9, 0.6)])
        return w, 7 + (d - 7) // 3, True
    if name == "ortol_pairs":
        w = np.concatenate([[1.0, 0.9, 0.9 + 3e-6, 0.8, 0.8 + 3e-5], _fill(rng, d - 5, -0.9, 0.6)])
        return w, 5 + (d - 5) // 3, True
    if name == "lowrank_6":
        return np.concatenate([_fill(rng, d - 6, 0.2, 1.0), np.zeros(6)]), d - 6, True
    if name == "lowrank_flip":
        nz = (3 * d) // 8
        return np.concatenate([_fill(rng, d - nz, 0.2, 1.0), np.zeros(nz)]), d - nz, False
    if name == "graded":
        return 2.0 ** (-40.0 * np.arange(d) / d), d // 8, False
    raise KeyError(name)


FAMILY = {"mult_33322": 1, "mult_6": 1, "mult_16": 1,
          "tight4_1e-7": 2, "tight6_1e-7": 2, "tight6_1e-11": 2, "ortol_pairs": 2,
          "lowrank_6": 3, "lowrank_flip": 3,
          "graded": 4,
          "diag_repeated": 5, "diag_mult_16": 5, "block_diag": 5, "wilkinson": 5, "wilkinson_glued": 5,
          "mult_33322_up": 6, "mult_33322_down": 6}
CASES = tuple(FAMILY)


def _assemble(Q, w):
    """A = Q diag(w) Q^H in long double, hermitised, rounded to complex128."""
    A = (Q * w.astype(LD)[None, :]) @ Q.conj().T
    A = (A + A.conj().T) / 2
    A = A.astype(np.complex128)
    return (A + A.conj().T) / 2


def _finish(name, A, w, Q, keep, full_ok):
    """Sort descending, cut the groups, place tau mid-gap after the keep-th eigenvalue."""
    w = np.asarray(w, dtype=LD)
    order = np.argsort(-w, kind="stable")
    w, Q = w[order], np.asarray(Q)[:, order]
    d = len(w)
    sep = SEP * float(np.abs(w).max())
    cuts = [0] + [i for i in range(1, d) if w[i - 1] - w[i] >= sep] + [d]
    groups = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        gap = min(float(w[a - 1] - w[a]) if a > 0 else np.inf, float(w[b - 1] - w[b]) if b < d else np.inf)
        groups.append(Group(np.arange(a, b), np.ascontiguousarray(Q[:, a:b].astype(np.complex128)), gap))
    assert keep in cuts and 0 < keep < d, (name, keep)
    tau = float((w[keep - 1] + w[keep]) / 2)
    for x in (A, ):
        x.setflags(write=False)
    return Case(name, A, w.astype(np.float64), tuple(groups), tau, full_ok)


def _blocks(mats):
    n = sum(m.shape[0] for m in mats)
    out = np.zeros((n, n), dtype=mats[0].dtype)
    o = 0
    for m in mats:
        out[o:o + m.shape[0], o:o + m.shape[0]] = m
        o += m.shape[0]
    return out


@functools.lru_cache(maxsize=None)
def _wilkinson_block(n, glued):
    T = wilkinson(n)
    if glued:   # two copies joined by one small off-diagonal entry
        T = _blocks([T, T])
        T[n - 1, n] = T[n, n - 1] = 1e-7
    w, U = jacobi_ld(T)
    return T, w, U


@functools.lru_cache(maxsize=None)
def case(name, d, seed=0):
    base = name[:-3] if name.endswith("_up") else name[:-5] if name.endswith("_down") else name
    rng = np.random.default_rng([d, seed, CASES.index(base)])     # (family 6: family 1's matrix, scaled)
    if name in ("diag_repeated", "diag_mult_16"):     # exactly diagonal: every reflector has tau = 0, every e = 0
        w, keep, full_ok = _spectrum(name, d, rng)
        w = w[rng.permutation(d)]
        return _finish(name, np.diag(w).astype(np.complex128), w, np.eye(d), keep, full_ok)
    if name == "block_diag":        # three blocks; 0.9 is an eigenvalue of each, 0.8 twice of the first
        sizes = (d // 3, d // 3, d - 2 * (d // 3))
        ws = [np.concatenate([[0.9, 0.8, 0.8], _fill(rng, sizes[0] - 3, -0.9, -0.3)]),
              np.concatenate([[0.9, 1.0], _fill(rng, sizes[1] - 2, -0.3, 0.2)]),
              np.concatenate([[0.9], _fill(rng, sizes[2] - 1, 0.2, 0.7)])]
        Qs = [unitary(n, seed + 1 + i) for i, n in enumerate(sizes)]
        A = _blocks([_assemble(Q, w) for Q, w in zip(Qs, ws)])
        return _finish(name, A, np.concatenate(ws), _blocks(Qs), 6, True)
    if name in ("wilkinson", "wilkinson_glued"):   # tridiagonal block next to a diagonal one (e = 0 from there on)
        glued = name == "wilkinson_glued"
        n = 21 if not glued or d >= 64 else 15
        T, wt, U = _wilkinson_block(n, glued)
        nf = d - T.shape[0]
        f = -2.0 - 10.0 * (np.arange(nf) + 0.5) / nf
        A = _blocks([T, np.diag(f)]).astype(np.complex128)
        w = np.concatenate([wt, f.astype(LD)])
        Q = _blocks([U, np.eye(nf, dtype=LD)])
        sw = np.sort(np.asarray(wt, dtype=float))[::-1]
        keep = int(np.sum(sw > 2.5))     # mid-gap of the W+ spectrum (2.96 | 2.13)
        return _finish(name, A, w, Q, keep, True)
    scale = {"mult_33322_up": 2.0 ** 100, "mult_33322_down": 2.0 ** -100}.get(name, 1.0)
    w, keep, full_ok = _spectrum(name, d, rng)
    A = _assemble(unitary(d, seed), w) * scale
    return _finish(name, A, w.astype(LD) * LD(scale), unitary(d, seed), keep, full_ok)


def random_hermitian(d, seed):
    """A GUE-like matrix through the same construction (distinct eigenvalues, neighbours >= SEP ||A|| apart)."""
    rng = np.random.default_rng([d, seed, 99])
    w = _fill(rng, d, -1.0, 1.0)
    return _finish("random", _assemble(unitary(d, seed), w), w, unitary(d, seed), max(1, d // 2), True)


def small_mult(d):
    """Family 1 at any order d >= 3: (3, 3, 3, 2, 2, distinct ...) from d = 31, one or two double eigenvalues below."""
    if d >= 31:
        return case("mult_33322", d)
    rng = np.random.default_rng([d, 0, 98])
    mult = (2, 2) if d >= 5 else (2,)
    w = _spec_mult(rng, d, mult)
    return _finish("mult_small", _assemble(unitary(d, 0), w), w, unitary(d, 0), sum(mult), True)


# ---------------------------------------------------------------- the checker
def _subspace_dist(Vg, Qg):
    a = Vg - Qg @ (Qg.conj().T @ Vg)
    b = Qg - Vg @ (Vg.conj().T @ Qg)
    return max(np.linalg.norm(a, 2), np.linalg.norm(b, 2))


def check(A, w, groups, lam, V, k, tau, margin=1.0):
    """Assert (EigCheckError) that (lam, V, k) is the decomposition of A on one side of tau.  V holds eigenvector q
    as row q.  k >= 0: the k eigenpairs above tau, descending; k < 0: the -k at or below it, ascending.  Returns the
    worst error / bound of every check."""
    d = A.shape[0]
    nrm = np.linalg.norm(A)
    n_above = int(np.sum(w > tau))
    side = k < 0
    kc = -int(k) if side else int(k)
    if kc != (d - n_above if side else n_above):
        raise EigCheckError("count", f"k = {k}, {n_above} of {d} eigenvalues lie above tau")
    rows = d - 1 - np.arange(kc) if side else np.arange(kc)      # positions in the descending spectrum
    ratios = {"eig": 0.0, "orth": 0.0, "res": 0.0, "shrunk": 0.0, "proj": 0.0}
    lk, Vk = np.asarray(lam[:kc], dtype=float), np.asarray(V[:kc]).T      # columns = eigenvectors
    s = np.where(w > tau, w - tau, 0.0)
    Xr = np.zeros((d, d), np.complex128)
    for g in groups:
        if s[g.idx[0]] > 0:
            Xr += (g.basis * s[g.idx][None, :]) @ g.basis.conj().T
    if side:
        X = A - tau * np.eye(d) + (Vk * (tau - lk)[None, :]) @ Vk.conj().T
    else:
        X = (Vk * (lk - tau)[None, :]) @ Vk.conj().T
    ratios["shrunk"] = np.linalg.norm(X - Xr) / (TOL * nrm)
    if kc:
        ratios["eig"] = np.abs(lk - w[rows]).max() / (TOL * nrm)
        ratios["orth"] = np.abs(Vk.conj().T @ Vk - np.eye(kc)).max() / ORTH
        ratios["res"] = np.linalg.norm(A @ Vk - Vk * lk[None, :], axis=0).max() / (TOL * nrm)
        pos = np.full(d, -1)
        pos[rows] = np.arange(kc)
        for g in groups:
            if len(g.idx) == d or pos[g.idx[0]] < 0:
                continue
            assert (pos[g.idx] >= 0).all(), "tau cuts a group"
            ratios["proj"] = max(ratios["proj"], _subspace_dist(Vk[:, pos[g.idx]], g.basis) / (TOL * nrm / g.gap))
    for which in ("eig", "orth", "res", "shrunk", "proj"):
        if not ratios[which] <= margin:     # (a NaN fails)
            raise EigCheckError(which, f"error / bound = {ratios[which]:.3g} (margin {margin})")
    return ratios


def check_case(c, lam, V, k, tau, margin=1.0):
    return check(c.A, c.w, c.groups, lam, V, k, tau, margin)
