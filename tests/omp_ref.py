"""Extended-precision reference of the batched OMP (csrc/ace_omp.hip), its parity cases and their tolerances.

The reference is the textbook loop

    r = y, I = {}
    repeat: stop if |I| = kmax or ||r||_2 <= tol
            j = argmax over j not in I of w_j |d_j^H r|^2        (ties: smaller j)
            I <- I u {j};  c = argmin ||y - D_I c||_2;  r = y - D_I c

in numpy longdouble (x87 extended, u_ld = 2^-64; mpmath would be far too slow for the 60 M complex products of the
largest case).  Every step's least-squares problem is solved afresh, not progressively: an f64 LAPACK solve of
the whole D_I, refined three times against the longdouble residual (each round contracts the error by about
kappa^2 u, 1e-10 at the kappa <= 1e3 of the cases, down to the longdouble floor).  Per step it records the selection
margin, ||r|| and kappa_2(D_I).

A run with tolerance tol is a prefix of the run with tol = 0 (the greedy path does not depend on the stopping rule),
so one trajectory per (case, colscale) serves the count mode and the tolerance mode: the tolerance is put half-way
between two consecutive residual norms of the trajectory.

Tolerances (derived from the kernel's least-squares method, with kappa and the norms from the reference).  The kernel
grows a QR factorisation of D_I by modified Gram-Schmidt and applies the same projections to the right-hand side
(z_k = q_k^H r, r -= z_k q_k), which is MGS on the augmented matrix [D_I y]: backward stable for least squares
(Bjorck 1967; Higham, Accuracy and Stability, Thm 20.4): the computed c is the exact solution for D_I + E, y + f with
||E|| <= eps ||D_I||, ||f|| <= eps ||y||.  eps: an entry of a column passes through a complex dot product of length d
(at most (d + 2) roundings per product term, a factor 2 sqrt(2) < 4 for complex arithmetic in norm) and through at
most k subtractions of a product (2 roundings each): 4 (d + 2 k + 2) u per column; twice that for perturbing both
D_I and y:

    eps = 8 (d + 2 k + 2) u,   u = 2^-53.

First-order perturbation theory of least squares (Higham Thm 20.1) then gives, with kappa = kappa_2(D_I),
smax = ||D_I||_2, for the coefficient vector and the residual

    ||c^ - c||_2   <= eps (kappa (||c|| + ||y|| / smax) + kappa^2 ||r|| / smax)
    | ||r^|| - ||r|| | <= ||r^ - r|| <= eps (smax ||c|| + ||y|| + kappa ||r||).

Conditions under which a bit-different f64 implementation must pick the same atoms (asserted for EVERY realisation of
every case in tests/test_omp_ref.py):
  1. at every selection the relative gap between the best and second-best weighted correlation is >= 1e-6;
  2. at every selection ||r|| >= 1e-6 ||y||;
  3. at every stopping decision | ||r|| - tol | >= 1e-6 tol;
  4. kappa_2(D_I) <= 1e3 throughout.
"""
import functools
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "2ace-mmwave-channel-estimation_amd"))

LD = np.longdouble
CLD = np.clongdouble
U = 2.0 ** -53

# (batch, d, N, kmax)
SHAPES = [(1, 1, 1, 1), (3, 5, 7, 5), (17, 16, 64, 3), (33, 17, 130, 8), (16, 64, 300, 16), (5, 130, 2401, 40),
          (2, 256, 1000, 128)]
TWO_STAGE = "two-stage-C"   # the extra case: C of sparse.two_stage_setup at 8 x 8, M = 48 (columns not unit-norm)
SEEDS = {}                  # shape -> seed where the default (0) breaches a condition


def model(D, y, kmax, tol=0.0, w=None, *, conj=True, select="abs2", exclude=True, coef="ls", dtype=np.complex128):
    """OMP of one realisation in ``dtype`` (complex128: a plain f64 model; clongdouble: the reference, refined).
    The switches make the four wrong models of tests/test_gpu_omp.py.  Returns a dict: idx, coef (final), norms
    [count + 1] (||r|| before each selection and at the end), margins, kappas, coefs (per step)."""
    ext = dtype is CLD
    rt = LD if ext else np.float64
    D64 = np.asarray(D, np.complex128)
    Dx = D64.astype(dtype)
    DH = np.ascontiguousarray(Dx.conj().T if conj else Dx.T)
    yx = np.asarray(y).astype(dtype)
    wx = np.ones(D.shape[1], rt) if w is None else np.asarray(w).astype(rt)
    r = yx.copy()
    I, norms, margins, kappas, coefs = [], [], [], [], []
    c = np.zeros(0, dtype)
    while True:
        nr = np.sqrt(np.sum(r.real * r.real + r.imag * r.imag))
        norms.append(nr)
        if len(I) == kmax or nr <= tol:
            break
        g = DH @ r
        v = (g.real * g.real if select == "real" else g.real * g.real + g.imag * g.imag) * wx
        if exclude and I:
            v[I] = -1
        j = int(np.argmax(v))              # (the first of equal maxima: the smaller index)
        rest = np.delete(v, j)
        margins.append(float((v[j] - rest.max()) / v[j]) if rest.size and v[j] > 0 else 1.0)
        if j in I:                         # (only without exclusion: a wrong model that stalls)
            break
        I.append(j)
        DI64 = D64[:, I]
        sv = np.linalg.svd(DI64, compute_uv=False)
        kappas.append(float(sv[0] / sv[-1]) if sv[-1] > 0 else np.inf)
        if coef == "corr":
            c = np.concatenate([c, [g[j]]])
            r = yx - Dx[:, I] @ c
        else:
            c = np.linalg.lstsq(DI64, np.asarray(yx, np.complex128), rcond=None)[0].astype(dtype)
            r = yx - Dx[:, I] @ c
            for _ in range(3 if ext else 0):
                c = c + np.linalg.lstsq(DI64, r.astype(np.complex128), rcond=None)[0].astype(dtype)
                r = yx - Dx[:, I] @ c
        coefs.append(c.copy())
    return {"idx": I, "coef": c, "norms": norms, "margins": margins, "kappas": kappas, "coefs": coefs}


def _cn(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)) * np.sqrt(0.5)


def _inputs(shape):
    """(D [d][N], Y [batch][d], w [N]): a complex Gaussian dictionary with unit columns, signals with
    min(kmax, max(1, kmax // 2 + 1)) atoms plus noise 0.05 ||signal|| / sqrt(d) per entry, colscale in [0.5, 1.5]."""
    if shape == TWO_STAGE:
        from ace_amd import sparse, synth
        AD = sparse.dictionary_2d(8, 8)[0]
        D = sparse.two_stage_setup(synth.codebook(7, 48, 64) @ AD, 3).C
        batch, kmax = 4, 6
        rng = np.random.default_rng([SEEDS.get(shape, 0), 99])
    else:
        batch, d, N, kmax = shape
        rng = np.random.default_rng([SEEDS.get(shape, 0), *shape])
        D = _cn(rng, d, N)
        D = D / np.sqrt(np.sum(np.abs(D) ** 2, axis=0))
    d, N = D.shape
    ns = min(kmax, N, max(1, kmax // 2 + 1))
    Y = np.empty((batch, d), np.complex128)
    for b in range(batch):
        sup = rng.choice(N, ns, replace=False)
        amp = (1.0 + rng.random(ns)) * np.exp(2j * np.pi * rng.random(ns))
        sig = D[:, sup] @ amp
        Y[b] = sig + 0.05 * np.linalg.norm(sig) / np.sqrt(d) * _cn(rng, d)
    return np.ascontiguousarray(D), Y, 0.5 + rng.random(N), kmax


@functools.lru_cache(maxsize=None)
def case(shape, scaled):
    """The inputs of a parity case and its reference trajectories (tol = 0, kmax atoms), computed once and shared:
    D, Y, w (None when not ``scaled``), kmax, traj [batch]."""
    D, Y, w, kmax = _inputs(shape)
    w = w if scaled else None
    traj = [model(D, Y[b], kmax, 0.0, w, dtype=CLD) for b in range(Y.shape[0])]
    for a in (D, Y):
        a.setflags(write=False)
    return {"D": D, "Y": Y, "w": w, "kmax": kmax, "traj": traj}


def tol_for(c, ks=None):
    """The tolerance of the tolerance mode: one number for the batch (the C-ABI takes one), half-way between two
    consecutive residual norms of realisation 0's trajectory, at ks = ceil(kmax / 2) atoms by default."""
    t = c["traj"][0]
    ks = (c["kmax"] + 1) // 2 if ks is None else ks
    return float(0.5 * (t["norms"][ks - 1] + t["norms"][ks]))


def expected(c, tol):
    """Per realisation what OMP returns at (kmax, tol), read off the tol = 0 trajectory: count, idx, coef
    (longdouble), resnorm, and the derived tolerances tol_coef (2-norm over the coefficient vector), tol_res."""
    out = []
    kmax = c["kmax"]
    d = c["D"].shape[0]
    for b, t in enumerate(c["traj"]):
        k = 0
        while k < kmax and not t["norms"][k] <= tol:
            k += 1
        cf = t["coefs"][k - 1] if k else np.zeros(0, CLD)
        ny = float(t["norms"][0])
        if k:
            sv = np.linalg.svd(c["D"][:, t["idx"][:k]], compute_uv=False)
            smax, kap = float(sv[0]), float(sv[0] / sv[-1])
        else:
            smax, kap = 1.0, 1.0
        eps = 8.0 * (d + 2 * k + 2) * U
        nc, nr = float(np.sqrt(np.sum(np.abs(cf) ** 2))), float(t["norms"][k])
        out.append({"count": k, "idx": t["idx"][:k], "coef": cf, "resnorm": t["norms"][k], "kappa": kap,
                    "tol_coef": eps * (kap * (nc + ny / smax) + kap * kap * nr / smax),
                    "tol_res": eps * (smax * nc + ny + kap * nr)})
    return out


def conditions(c, tol):
    """The worst figures of the four conditions over the realisations of a case at tolerance tol: (smallest
    selection margin, smallest ||r|| / ||y|| at a selection, smallest | ||r|| - tol | / tol at a stopping decision
    (inf at tol = 0), largest kappa)."""
    gap, rel, stop, kap = np.inf, np.inf, np.inf, 0.0
    for e, t in zip(expected(c, tol), c["traj"]):
        k = e["count"]
        for i in range(k):
            gap = min(gap, t["margins"][i])
            rel = min(rel, float(t["norms"][i] / t["norms"][0]))
            kap = max(kap, t["kappas"][i])
        if tol > 0:
            for i in range(k + 1):
                stop = min(stop, abs(float(t["norms"][i]) - tol) / tol)
    return gap, rel, stop, kap


def ratios(c, tol, idx, coef, count, resnorm):
    """Worst err / tol of coef and resnorm over the batch (idx and count are compared exactly by the caller)."""
    qc = qr = 0.0
    for b, e in enumerate(expected(c, tol)):
        k = e["count"]
        dc = np.asarray(coef[b, :k]).astype(CLD) - e["coef"]
        qc = max(qc, float(np.sqrt(np.sum(np.abs(dc) ** 2))) / e["tol_coef"]) if k else qc
        qr = max(qr, abs(float(LD(resnorm[b]) - e["resnorm"])) / e["tol_res"])
    return {"coef": qc, "resnorm": qr}
