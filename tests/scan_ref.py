"""References and derived tolerances for the beam scan (ace_beam_scan_batch, csrc/ace_scan.hip):
tests/test_gpu_scan.py and tests/test_gpu_baselines.py compare against them, tests/test_scan_ref.py tests them on
the CPU.  Not collected.

    y[b][p][q] = sum_i sum_j conj(W0[q][i]) x_b[i + d0 j] F1[p][j]       (w' * H * f, MyBeamSweeping.m:109)
    P = |y + noise|^2,  f = p Q0 + q,  top-K by (P larger, then f smaller),  total = sum P

``scan``   the plain numpy (f64) restatement, with the deliberately wrong variants of tests/test_scan_ref.py.
``exact``  the reference.  Where the beams are Gaussian integers the product is evaluated without rounding
           (tests/linop_ref.py: the matrix kron(F1, conj W0), whose entries are then exact in f64, against x in
           sliced-integer planes, recombined in Python integers, returned as hi + lo).  Otherwise the two
           products run in numpy's longdouble (64-bit mantissa on x86: every rounding 2^-11 of the f64 unit
           roundoff, at most (d0 + d1) 2^-11 u S in all, below the tolerance by the factor 2^-11 / C_Y).  Noise,
           modulus, sums and the selection are in longdouble in both cases.

Tolerance of y (u = 2^-53, S_pq = sum_i sum_j |W0[q][i]| |x_ij| |F1[p][j]|, complex moduli)
-------------------------------------------------------------------------------------------
    tol_y = C_Y (d0 + d1 + 8) u (S_pq + |noise_pq|),      C_Y = 4.
The kernel chains two 3M products on the f64 matrix cores.  tests/rss_ref.py derives, for one 3M dot product of
length n with absolute sum S, a complex error of at most sqrt(10) (n + 4) u S to first order (gamma_n on each of
the three real dot products, one rounding per pre-added factor, two subtractions on partial results of at most
3 S).  Here
    T_pi = sum_j F1[p][j] x_ij            |dT_pi| <= sqrt(10) (d1 + 4) u S1_pi,    S1_pi = sum_j |F1[p][j]| |x_ij|
    y_pq = sum_i conj(W0[q][i]) T^_pi     (the conjugation is a sign flip: exact)
          its own rounding                <= sqrt(10) (d0 + 4) u sum_i |W0[q][i]| |T^_pi| <= sqrt(10) (d0 + 4) u S_pq (1 + O(u))
          the error carried in from T     <= sum_i |W0[q][i]| |dT_pi|              <= sqrt(10) (d1 + 4) u S_pq
so |dy| <= 3.17 (d0 + d1 + 8) u S_pq.  Adding the noise rounds each component once more, at most sqrt(2) u
|y + noise| <= 1.42 u (S_pq + |noise_pq|); against the 0.83 (d0 + d1 + 8) >= 8.3 that C_Y = 4 leaves, this and the
second-order terms ((d0 + d1) u < 2^-46) are covered.  The numpy restatement (4M products, gamma_2n sqrt(2) S each)
lies inside the same bound.

Propagation (z = y + noise exact, delta = tol_y, N = Q0 Q1)
-----------------------------------------------------------
    tol_P     = 2 |z| delta + delta^2 + 3u P        (the two squares and their sum: (1 + u)^2 - 1 < 3u)
    tol_total = sum tol_P + N u sum P               (N - 1 additions in any order)
top_idx is compared exactly: ``gaps`` states the precondition (the reference powers around the cut are further
apart than any rounding), and the status word and the values of degenerate realisations are exact as well.
"""
import functools
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import linop_ref as LR  # noqa: E402

U = 2.0 ** -53
C_Y = 4.0
ST_DEGENERATE = 256
LD, CLD = np.longdouble, np.clongdouble

# (batch, d0, d1, Q0, Q1, K) of the GPU parity suite: the minimum; K-loop tails on both products; the 16-antenna
# dictionary; full tiles and several work-groups; the 32-antenna dictionary with masked beam tiles; the largest map
# with K at its cap; odd everything with Q0 != Q1 (three W0 tiles, the last one masked); a 1-D scan
SHAPES = [(1, 1, 1, 1, 1, 1), (3, 3, 5, 7, 2, 3), (5, 16, 16, 49, 49, 1), (17, 16, 16, 64, 64, 4),
          (2, 32, 32, 95, 95, 3), (65, 32, 32, 128, 128, 16), (4, 17, 31, 130, 33, 5), (3, 32, 1, 20, 1, 2)]
KINDS = ("random", "phase")
MODELS = ("no_conj_w", "conj_f", "flat_qp", "modulus")


def _mat(X, d0, d1):
    """[batch][i][j] = x[i + d0 j]."""
    X = np.atleast_2d(X)
    return X.reshape(X.shape[0], d1, d0).transpose(0, 2, 1)


def scan(X, W0, F1, noise=None, model=None):
    """numpy f64 restatement: the power map [batch][Q1*Q0] in flat order f = p Q0 + q.  ``model``: one of MODELS."""
    W0, F1 = np.atleast_2d(np.asarray(W0, np.complex128)), np.atleast_2d(np.asarray(F1, np.complex128))
    (Q0, d0), (Q1, d1) = W0.shape, F1.shape
    H = _mat(np.asarray(X, np.complex128), d0, d1)
    Wc = W0 if model == "no_conj_w" else W0.conj()
    Fc = F1.conj() if model == "conj_f" else F1
    y = np.matmul(Wc[None], np.matmul(H, Fc.T[None])).transpose(0, 2, 1)   # [b][p][q] (two zgemms)
    if model == "flat_qp":
        y = y.transpose(0, 2, 1)
    y = y.reshape(H.shape[0], Q0 * Q1)
    if noise is not None:
        y = y + np.asarray(noise, np.complex128).reshape(y.shape)
    a = np.abs(y)
    return a if model == "modulus" else a * a


def _gaussian_integers(A):
    r = np.ascontiguousarray(A).view(np.float64)
    return bool(np.all(r == np.rint(r)) and np.all(np.abs(r) < 2 ** 20))


def product(X, W0, F1):
    """y [batch][Q1][Q0] as (re, im) longdouble arrays: exact (hi + lo of the integer-plane product) for
    Gaussian-integer beams, else accumulated in longdouble."""
    (Q0, d0), (Q1, d1) = W0.shape, F1.shape
    X = np.atleast_2d(np.asarray(X, np.complex128))
    if _gaussian_integers(W0) and _gaussian_integers(F1):
        A = (F1[:, None, :, None] * W0.conj()[None, :, None, :]).reshape(Q1 * Q0, d1 * d0)   # [p Q0 + q][i + d0 j]
        hi, lo = LR.exact_cmatvec(A, X)
        re = hi[:, 0::2].astype(LD) + lo[:, 0::2].astype(LD)
        im = hi[:, 1::2].astype(LD) + lo[:, 1::2].astype(LD)
        return re.reshape(-1, Q1, Q0), im.reshape(-1, Q1, Q0)
    H = _mat(X, d0, d1).astype(CLD)
    T = np.matmul(H, F1.astype(CLD).T[None])                       # [b][i][p]
    y = np.matmul(T.transpose(0, 2, 1), W0.conj().astype(CLD).T[None])   # [b][p][q]
    return y.real, y.imag


def select(P, K):
    """(top_pow, top_idx) [batch][K] of a flat power map by the order (P larger, then f smaller)."""
    batch, N = P.shape
    idx = np.empty((batch, K), np.int32)
    for b in range(batch):
        idx[b] = np.lexsort((np.arange(N), -P[b]))[:K]   # (last key first: by -P, ties by f)
    return np.take_along_axis(P, idx.astype(np.int64), axis=1), idx


def exact(X, W0, F1, K, noise=None, yparts=None):
    """Exact reference and tolerances: a dict with ``power`` [batch][Q1*Q0], ``top_pow`` [batch][K], ``total``
    [batch] (longdouble), ``top_idx`` [batch][K] int32, ``sorted`` (each realisation's K + 1 largest powers),
    ``tol_power``, ``tol_total`` (f64) and ``status``.  Inputs must be finite.  ``yparts``: a ``product`` result
    to reuse."""
    W0, F1 = np.atleast_2d(np.asarray(W0, np.complex128)), np.atleast_2d(np.asarray(F1, np.complex128))
    X = np.atleast_2d(np.asarray(X, np.complex128))
    (Q0, d0), (Q1, d1) = W0.shape, F1.shape
    batch, N = X.shape[0], Q0 * Q1
    re, im = product(X, W0, F1) if yparts is None else yparts
    re, im = re.reshape(batch, N), im.reshape(batch, N)
    S = np.matmul(np.abs(W0)[None], np.matmul(np.abs(_mat(X, d0, d1)), np.abs(F1).T[None])).transpose(0, 2, 1).reshape(batch, N)
    if noise is not None:
        nz = np.asarray(noise, np.complex128).reshape(batch, N)
        re, im = re + nz.real.astype(LD), im + nz.imag.astype(LD)
        S = S + np.abs(nz)
    P = re * re + im * im
    delta = C_Y * (d0 + d1 + 8) * U * S
    Pf = P.astype(np.float64)
    tol_power = 2 * np.sqrt(Pf) * delta + delta * delta + 3 * U * Pf
    top_pow, top_idx = select(P, K)
    srt = -np.sort(-P, axis=1)[:, :K + 1]
    return {"power": P, "top_pow": top_pow, "top_idx": top_idx, "total": P.sum(axis=1), "sorted": srt,
            "tol_power": tol_power, "tol_total": tol_power.sum(axis=1) + N * U * Pf.sum(axis=1),
            "status": np.zeros(batch, np.uint32)}


def gaps(ref, K):
    """The smallest relative gap (P_r - P_{r+1}) / P_r between consecutive reference powers among ranks 1 .. K + 1,
    over the realisations (inf when the map has a single entry; 0 for a tie)."""
    s = ref["sorted"][:, :K + 1]
    if s.shape[1] < 2:
        return float("inf")
    a, b = s[:, :-1], s[:, 1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(a > 0, (a - b) / a, 0)
    return float(g.min())


def ratios(ref, power=None, top_pow=None, total=None):
    """Worst err / tol of whichever outputs are given against ``exact``'s dict.  The tolerance of a top_pow entry
    is that of the map entry the reference selects there (top_idx is the caller's exact comparison)."""
    out = {}

    def worst(got, want, tol):
        e = np.abs(np.asarray(got, np.float64).astype(LD).reshape(want.shape) - want).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(e == 0, 0.0, e / tol)
        return float(np.max(q)) if q.size else 0.0

    if power is not None:
        out["power"] = worst(power, ref["power"], ref["tol_power"])
    if top_pow is not None:
        tol = np.take_along_axis(ref["tol_power"], ref["top_idx"].astype(np.int64), axis=1)
        out["top_pow"] = worst(top_pow, ref["top_pow"], tol)
    if total is not None:
        out["total"] = worst(total, ref["total"], ref["tol_total"])
    return out


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def beams(rng, kind, Q, d):
    """"random": complex normals with full mantissas; "phase": c (+-1, +-j) with c = 1 / sqrt(d)."""
    if kind == "random":
        return rng.standard_normal((Q, d)) + 1j * rng.standard_normal((Q, d))
    return (1j ** rng.integers(0, 4, (Q, d))) * (1.0 / np.sqrt(d))


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """Seeded inputs of one parity case with their exact references, without and with noise (computed once,
    shared, read-only): x with a per-realisation scale over 2^+-8, noise CN(0, 0.1 mean |y_b|^2)."""
    batch, d0, d1, Q0, Q1, K = shape
    rng = np.random.default_rng([*shape, KINDS.index(kind)])
    W0, F1 = beams(rng, kind, Q0, d0), beams(rng, kind, Q1, d1)
    X = ((rng.standard_normal((batch, d0 * d1)) + 1j * rng.standard_normal((batch, d0 * d1)))
         * np.exp2(rng.uniform(-8, 8, (batch, 1))))
    g = rng.standard_normal((batch, Q1 * Q0)) + 1j * rng.standard_normal((batch, Q1 * Q0))
    noise = g * np.sqrt(0.05 * scan(X, W0, F1).mean(axis=1))[:, None]
    yparts = product(X, W0, F1)
    ref = exact(X, W0, F1, K, None, yparts)
    ref_n = exact(X, W0, F1, K, noise, yparts)
    _freeze(X, W0, F1, noise, *ref.values(), *ref_n.values())
    return {"X": X, "W0": W0, "F1": F1, "noise": noise, "K": K, "ref": ref, "ref_noise": ref_n}


def tie_case(all_equal=False):
    """Exact ties: Gaussian-integer x, beams in {0, +-1, +-j} with duplicated rows in W0 and in F1, integer noise:
    every product is exact in f64, so the power map is exact and tied pairs must come out smaller index first.
    (batch, d0, d1, Q0, Q1) = (4, 5, 3, 9, 6), K = 16.  ``all_equal``: x_ij = 1 and every beam a single 1, no noise:
    all Q0 Q1 powers are 1."""
    rng = np.random.default_rng(77)
    batch, d0, d1, Q0, Q1, K = 4, 5, 3, 9, 6, 16
    if all_equal:
        X = np.ones((batch, d0 * d1), np.complex128)
        W0 = np.zeros((Q0, d0), np.complex128)
        W0[np.arange(Q0), np.arange(Q0) % d0] = 1
        F1 = np.zeros((Q1, d1), np.complex128)
        F1[np.arange(Q1), np.arange(Q1) % d1] = 1
        noise = None
    else:
        gi = lambda *s: rng.integers(-1, 2, s) * (1j ** rng.integers(0, 2, s))   # noqa: E731  {0, +-1, +-j}
        X = (rng.integers(-9, 10, (batch, d0 * d1)) + 1j * rng.integers(-9, 10, (batch, d0 * d1))).astype(np.complex128)
        W0, F1 = gi(Q0, d0).astype(np.complex128), gi(Q1, d1).astype(np.complex128)
        W0[[4, 7]] = W0[[1, 1]]       # duplicated rows: tied pairs (p, 1), (p, 4), (p, 7) for every p
        F1[[3, 5]] = F1[[0, 2]]
        noise = (rng.integers(-1, 2, (batch, Q1 * Q0)) + 0j)
        noise[:, ::2] = 0
        noise[1] = 0                  # a realisation whose duplicated rows tie exactly
    ref = exact(X, W0, F1, K, noise)
    return {"X": X, "W0": W0, "F1": F1, "noise": noise, "K": K, "ref": ref}
