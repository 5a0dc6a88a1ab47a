"""Longdouble references, inputs and derived tolerances for the kernels of the r-column stages and of the pipeline
around them (csrc/ace_stage.hip; tests/test_gpu_stage.py, self-tested on the CPU by tests/test_stage_ref.py).

The references are line-by-line transcriptions of inferLowRankV4_multi.m in numpy longdouble (64-bit mantissa: the
reference's own rounding is 2^-11 u, u = 2^-53) -- mpmath for the eigenproblem of the rotation -- on the f64 inputs
taken exactly:

    :296-310  init: scale X by norm(B) / norm(A X) (row mode: Frobenius; column mode: per column), Y = normalize_rows
    :511-533  ArgMinY (row / column mode, the D == 0 rows)          :336-337  M += mu (A X - Y)
    :336-361  the sums of the iteration and the best-objective test (per-column objective, first minimiser)
    :263-264  [V, ~] = eig(X' X); X = X V (ascending, not re-sorted)
    :68       quality = 1 - norm(abs(A_test X) - B_test) / norm(B_test)
    :79-107   best of restarts, rollback on similarity < 0.6 when the last quality > 0.6, rescale by B_norm / A_norm
    :384-385  opt_X / opt_Y

Elementwise outputs
-------------------
Each carries a first-order running error bound built from the kernel's operations, every operation +, -, *, /, sqrt
contributing one relative u (a fused multiply-add contributes less, never more):
  init   nB = sqrt(sum B^2): (m + 1) u on the sum, half of it and one u after the root.  sum |P0|^2: (m + r + 2) u.
         scale = nB / sqrt(.): e_s = (m + r/2 + 5) u.  X = X0 scale: gamma(e_s + 1) |X| per component.  A X = P0 scale,
         D from its squares ((r + 2) u, halved, + u), B / D and the product: gamma(2 e_s + r/2 + 6) |Y| per component.
         Zero rows are exact: B_i / sqrt(r) (row mode, fl(1 / fl(sqrt(r))) B_i) and B_i (column mode): compared bit for bit.
  Y-step AX = S - g: u |AX|;  C = AX + M (1/mu): u |AX| + 2u |M/mu| + u |C|; then D, B / D, f = (B/D + mu) / (1 + mu),
         Y = C f, J = AX - Y and M' = M + mu J by the chain rule on those bounds (``ystep_ref`` spells each line).
Copies, gathers, scatters and selections, finish's x (B_norm / A_norm) and the zero-row values are compared bit for bit
with a numpy f64 restatement (one f64 operation each, correctly rounded on both sides).

Reductions
----------
A sum of N terms in any order is within gamma_(N-1) sum |terms| (Higham (4.4)); a term that is a squared modulus
adds 3 operations, and the rounding of its argument enters as 2 |x| dx.  nB, nAX2, nY2, nJM2, dY2 and the objectives
use k = N + 3.  quality: the dot product a_i x is within gamma_(2n+1) sum_k (|a_r x_r| + |a_i x_i|) per component, the
modulus adds (|re| e_re + |im| e_im) / |z| + 2u |z|, d = |z| - b one u, d^2 -> 2 |d| e_d + u d^2, the sequential sum
over the test rows gamma_mte; the two square roots halve the relative error of their argument and add one u each (at
sum = 0 the absolute error is sqrt of the sum's bound), the quotient and the final 1 - . one u each:
    e_q = [ e_s0 + rho (gamma_(mte+1) / 2 + 2u) ] + u |q|,   rho = s0 / s1,  e_s0 = e_v0 / (2 s0) + u s0.

part_gfix
---------
The reference is the exact function of the kernel's inputs, g_t = u_t - sum_e conj(G[e][t]) (geinv u_e)_e and 0 on the
test rows; each of the two fixed-order complex sums over te terms is within gamma_(2te+2) sum |a||b| per component,
the first one's error passes through |G|, and the subtraction adds u |g|.
The Schur identity is checked apart: with G~ = fl((I + K)^-1) and geinv = G~_ee^-1 the function equals S(G~) T_t for any
T~ on the test rows, S the Schur complement.  S(G~) - (I + K_t)^-1 = dS with ||dS|| <= ||dG|| (1 + ||W||)^2,
W = B_tt^-1 B_te, ||W|| <= sqrt(||B||) (B = I + K HPD, lambda_min(B_tt) >= 1), ||dG||_2 <= u sqrt(m) ||G||_2 <= u sqrt(m):
    || g - (I + K_t)^-1 T_t ||_2 <= u kappa(I + K) [ 4 sqrt(m) ||T_t|| + 4 te ||T~|| ]
(the second term: geinv is rounded to f64, |dX| <= u |X| with ||X||_2 <= kappa, so up to u te kappa ||T~|| of the
test rows' T~ is left uncancelled).

part_geinv
----------
The reference inverse is longdouble Gauss-Jordan with partial pivoting and Newton refinement, accepted when
max |G_ee X - I| <= 1e-17.  The kernel's bound is c te u kappa_2(G_ee) ||X||_2 on max |X^ - X|; c is not derivable
tightly: tests/test_stage_ref.py measures the largest err / (te u kappa ||X||) of ``gj_f64`` (the kernel's unpivoted
elimination order in numpy f64) over the suite's inputs, asserts it below GJ_RATIO, and the kernel gets 4 GJ_RATIO
(it differs from that restatement by fma contraction and the form of the complex multiply).

gram_rotate
-----------
Compared phase-free against the mp eigenpairs (lam, v) of the exactly formed Gram matrix H = X^H X:
  (a) ||Xout Xout^H - X X^H||_F <= [2 (2 32 + 2) sqrt(r) + 8 ORTH r] u ||X||_F^2: the two 32-wide products plus the
      eigenvectors' departure from unitarity;
  (b) max_{i != j} |Xout^H Xout|_ij / sqrt(d_i d_j) in units of u kappa(H) (over the non-null columns);
  (c) column norms ascending, | ||xout_k||^2 - lam_k | in units of u ||H||;
  (d) ||xout_k - e^{j t} X v_k|| in units of u ||H|| ||X||_2 / gap_k;
(c), (d) where the relative gap is at least 1e-3.  The multipliers of (b)-(d) and ORTH depend on the eigensolver: the
f64 oracle (numpy.linalg.eigh on fl(X^H X)) is measured against the mp reference on the suite's inputs, the figures
are recorded in GRAM_ORACLE and the kernel gets 8 x them.  Rank-deficient inputs: (a), (b) and the null columns' norms
at most sqrt(u) ||X||_2 only.

Decisions (qlast > 0.6, sim < 0.6, qmax < q, the first argmin of the column objective, the ascending order) are
compared exactly; every case's margin from equality is at least 1e-6 relative on the reference alone, except the cases
built to sit on the boundary (qlast == 0.6: no rollback; duplicated columns: the first index wins).
"""
import functools
import math

import mpmath as mp
import numpy as np

import zprox_ref as ZR

U = 2.0 ** -53
LD = np.longdouble
MARGIN = 1e-6
GAP = 1e-3
# largest err / (te u kappa_2 ||X||_2) of gj_f64 over GEINV_CASES, rounded up (measured 0.163 at te = 1;
# tests/test_stage_ref.py::test_gj_restatement_inside_ratio prints it)
GJ_RATIO = 0.25
GJ_MULT = 4.0
# the f64 oracle's figures over GRAM_CASES, rounded up (measured: orth 3.10, b 0.90, c 21.4, d 3.55;
# tests/test_stage_ref.py::test_gram_oracle_inside_ratios prints them); the kernel gets GRAM_MULT x
GRAM_ORACLE = {"orth": 3.2, "b": 1.0, "c": 22.0, "d": 3.6}
GRAM_MULT = 8.0
DPS = 40


def gam(k):
    return k * U / (1.0 - k * U)


def cx(x):
    """complex array -> longdouble array with a trailing (re, im) axis, exactly."""
    x = np.ascontiguousarray(np.asarray(x, np.complex128))
    return x.view(np.float64).reshape(x.shape + (2,)).astype(LD)


def err_over_tol(got, ref, tol):
    """max |got - ref| / tol per real component (got complex or real f64; ref, tol longdouble with the (re, im) axis
    for complex).  Where ref is NaN, got must be NaN (ratio 0), and nowhere else (ratio inf).  tol == 0 demands
    equality."""
    got = np.asarray(got)
    g = cx(got) if np.iscomplexobj(got) else got.astype(LD)
    ref, tol = np.broadcast_arrays(np.asarray(ref, LD), np.asarray(tol, LD))
    assert g.shape == ref.shape, (g.shape, ref.shape)
    if g.size == 0:
        return 0.0
    nan_r, nan_g = np.isnan(ref), np.isnan(g)
    if (nan_r != nan_g).any():
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(nan_r, 0, np.abs(g - ref))
        ratio = np.where(d == 0, 0, d / np.where(nan_r, 1, tol))
    return float(np.max(ratio))


# ---------------------------------------------------------------- init (:296-310)
def init_ref(X0, P0, B, row, mask=None):
    """X, Y of InferADMM's init given P0 = A X0 ([b][r][n], [b][r][m], [b][m]); mask [b][m]: 1 on the rows that take
    part.  Returns {name: (value, tol)} (longdouble, trailing (re, im) axis) and nB."""
    X0, P0, B = cx(X0), cx(P0), np.asarray(B, np.float64).astype(LD)
    b, r, m = P0.shape[:3]
    w = np.ones((b, m), LD) if mask is None else (np.asarray(mask) != 0).astype(LD)
    nB2 = np.sum(w * B * B, axis=1)
    nB = np.sqrt(nB2)
    cs = np.sum(w[:, None, :] * np.sum(P0 * P0, axis=-1), axis=2)                  # [b][r]
    s2 = np.broadcast_to(cs.sum(axis=1, keepdims=True), cs.shape) if row else cs
    scale = nB[:, None] / np.sqrt(s2)
    e_s = m + r / 2 + 5
    X = X0 * scale[:, :, None, None]
    ax = P0 * scale[:, :, None, None]
    a2 = np.sum(ax * ax, axis=-1)                                                  # [b][r][m]
    unit = np.zeros((b, r, m, 2), LD)
    Bb = np.broadcast_to(B[:, None, :], (b, r, m))
    if row:
        D = np.broadcast_to(np.sqrt(a2.sum(axis=1))[:, None, :], (b, r, m))
        unit[..., 0] = Bb / np.sqrt(LD(r))
    else:
        D = np.sqrt(a2)
        unit[..., 0] = Bb
    zero = D == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        Y = np.where(zero[..., None], unit, ax * (Bb / np.where(zero, 1, D))[..., None])
    Y = Y * w[:, None, :, None]
    out = {"X": (X, gam(e_s + 1) * np.abs(X)), "Y": (Y, gam(2 * e_s + r / 2 + 6) * np.abs(Y)),
           "nB": (nB, gam((m + 1) / 2 + 1) * nB)}
    return out, zero & (w[:, None, :] != 0)


def init_zero_rows_f64(B, r, row):
    """The kernel's value on a D == 0 row, restated in f64: (1 / sqrt(r)) B_i (row mode), B_i (column mode)."""
    B = np.asarray(B, np.float64)
    return (np.float64(1.0) / np.sqrt(np.float64(r))) * B if row else B.copy()


# ---------------------------------------------------------------- Y-step (:511-533, :336-361)
def ystep_ref(S, g, M, B, Yold, mu, row, mask=None):
    """One Y-step of every realisation: Y, M' with componentwise bounds, the five sums, the objective(s) and in
    column mode the first minimiser with its margin.  Arrays [b][r][m] c128, B [b][m], mu [b]."""
    S, g, M, Yo = cx(S), cx(g), cx(M), cx(Yold)
    B = np.asarray(B, np.float64).astype(LD)
    b, r, m = S.shape[:3]
    mu = np.asarray(mu, np.float64).astype(LD).reshape(b, 1, 1)
    w = np.ones((b, m), LD) if mask is None else (np.asarray(mask) != 0).astype(LD)
    w3, w4 = w[:, None, :], w[:, None, :, None]
    mu4 = mu[..., None]
    Bb = np.broadcast_to(B[:, None, :], (b, r, m))
    with np.errstate(invalid="ignore", divide="ignore"):
        ax = S - g
        e_ax = U * np.abs(ax)
        mm = M / mu4
        c = ax + mm
        e_c = e_ax + 2 * U * np.abs(mm) + U * np.abs(c)
        c2 = np.sum(c * c, axis=-1)
        ce = 2 * np.sum(np.abs(c) * e_c, axis=-1)
        if row:
            d2 = np.broadcast_to(c2.sum(axis=1)[:, None, :], (b, r, m))
            e_d2 = np.broadcast_to(ce.sum(axis=1)[:, None, :], (b, r, m)) + gam(r + 2) * d2
        else:
            d2, e_d2 = c2, ce + gam(3) * c2
        D = np.sqrt(d2)
        zero = D == 0
        Dz = np.where(zero, 1, D)
        e_D = np.where(zero, 0, e_d2 / (2 * Dz) + U * D)
        q = Bb / Dz
        e_q = Bb * e_D / (Dz * Dz) + U * np.abs(q)
        f = (q + mu) / (1 + mu)
        e_f = (e_q + U * np.abs(q + mu)) / (1 + mu) + 2 * U * np.abs(f)
        unit = np.zeros((b, r, m, 2), LD)
        unit[..., 0] = 1 / np.sqrt(LD(r)) if row else 1
        e_unit = np.zeros((b, r, m, 2), LD)
        e_unit[..., 0] = 2 * U if row else 0
        cc = np.where(zero[..., None], unit, c)
        e_cc = np.where(zero[..., None], e_unit, e_c)
        y = cc * f[..., None]
        e_y = np.abs(f)[..., None] * e_cc + np.abs(cc) * e_f[..., None] + U * np.abs(y)
        y, e_y = y * w4, e_y * w4
        jm = ax - y
        e_jm = e_ax + e_y + U * np.abs(jm)
        Mn = M + mu4 * jm
        e_M = mu4 * e_jm + U * np.abs(mu4 * jm) + U * np.abs(Mn)
        Mn = np.where(w4 != 0, Mn, M)
        e_M = e_M * w4
        k = r * m + 3

        def total(x, e_x):
            x, e_x = x * w4, e_x * w4
            v = np.sum(x * x, axis=(1, 2, 3))
            return v, gam(k) * v + 2 * np.sum(np.abs(x) * e_x, axis=(1, 2, 3))
        dy = y - Yo
        sums = {"nAX2": total(ax, e_ax), "nY2": total(y, e_y), "nJM2": total(jm, e_jm),
                "dY2": total(dy, e_y + U * np.abs(dy))}
        a2 = np.sum(ax * ax, axis=-1)
        e_a2 = 2 * np.sum(np.abs(ax) * e_ax, axis=-1)
        if row:
            a2, e_a2 = a2.sum(axis=1), e_a2.sum(axis=1)       # [b][m]
            e_a2 = e_a2 + gam(r + 2) * a2
            Bo, wo = B, w
        else:
            e_a2 = e_a2 + gam(3) * a2                         # [b][r][m]
            Bo, wo = Bb, np.broadcast_to(w3, (b, r, m))
        sa = np.sqrt(a2)
        e_sa = np.where(sa > 0, e_a2 / (2 * np.where(sa > 0, sa, 1)), 0) + U * sa
        o = sa - Bo
        e_o = e_sa + U * np.abs(o)
        o2 = o * o * wo
        e_o2 = (2 * np.abs(o) * e_o + U * o * o) * wo
        obj2 = o2.sum(axis=-1)
        e_obj2 = gam(m) * obj2 + e_o2.sum(axis=-1)
    out = {"Y": (y, e_y), "M": (Mn, e_M), **sums}
    if row:
        out["obj2"] = (obj2, e_obj2)
        return out, None
    objs = np.sqrt(obj2)                                      # [b][r]
    col = np.zeros(b, np.int64)
    margin = np.full(b, math.inf)
    for i in range(b):
        fin = np.flatnonzero(~np.isnan(objs[i]))
        if fin.size == 0:
            continue
        j = fin[np.argmin(objs[i][fin])]                      # (argmin returns the first minimiser)
        col[i] = j
        rest = [float((objs[i][t] - objs[i][j]) / objs[i][j]) for t in fin if t != j]
        margin[i] = min(rest) if rest else math.inf
    idx = np.arange(b)
    out["obj2"] = (obj2[idx, col], e_obj2[idx, col])
    return out, (col, margin)


# ---------------------------------------------------------------- quality (:68)
def quality_ref(A, X, B):
    """quality per realisation with its bound.  A [mte][n] (or [b][mte][n]: each realisation's own test rows),
    X [b][n], B [b][mte]."""
    X = np.asarray(X, np.complex128)
    b, n = X.shape
    A = np.asarray(A, np.complex128)
    if A.ndim == 2:
        A = np.broadcast_to(A, (b,) + A.shape)
    mte = A.shape[1]
    B = np.asarray(B, np.float64).astype(LD).reshape(b, mte)
    a, x = cx(A), cx(X)[:, None, :, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        re = np.sum(a[..., 0] * x[..., 0] - a[..., 1] * x[..., 1], axis=-1)
        im = np.sum(a[..., 0] * x[..., 1] + a[..., 1] * x[..., 0], axis=-1)
        e_re = gam(2 * n + 1) * np.sum(np.abs(a[..., 0] * x[..., 0]) + np.abs(a[..., 1] * x[..., 1]), axis=-1)
        e_im = gam(2 * n + 1) * np.sum(np.abs(a[..., 0] * x[..., 1]) + np.abs(a[..., 1] * x[..., 0]), axis=-1)
        mag = np.sqrt(re * re + im * im)
        e_mag = np.where(mag > 0, (np.abs(re) * e_re + np.abs(im) * e_im) / np.where(mag > 0, mag, 1),
                         e_re + e_im) + 2 * U * mag
        d = mag - B
        e_d = e_mag + U * np.abs(d)
        v0 = np.sum(d * d, axis=1)
        e_v0 = gam(mte) * v0 + np.sum(2 * np.abs(d) * e_d + U * d * d, axis=1)
        v1 = np.sum(B * B, axis=1)
        s0, s1 = np.sqrt(v0), np.sqrt(v1)
        e_s0 = np.where(s0 > 0, e_v0 / (2 * np.where(s0 > 0, s0, 1)), np.sqrt(e_v0)) + U * s0
        rho = s0 / s1
        q = 1 - rho
        e_q = e_s0 / s1 + rho * (gam(mte + 1) / 2 + 2 * U) + U * np.abs(q)
    return q, e_q


# ---------------------------------------------------------------- keep_best, finish, finalize_r: f64 restatements
def keep_best_f64(first, q, qmax, X, Y, Xmax, Ymax):
    """(:79-83) and the first restart's NaN seed.  Returns (qmax, Xmax, Ymax, better)."""
    q, qmax = np.asarray(q, np.float64), np.array(qmax, np.float64)
    Xm, Ym = np.array(Xmax, np.complex128), np.array(Ymax, np.complex128)
    better = qmax < q
    take = better | (bool(first) & np.isnan(q))
    Xm[take], Ym[take] = np.asarray(X)[take], np.asarray(Y)[take]
    qmax[better] = q[better]
    return qmax, Xm, Ym, better


def finish_ref(qlast, X, Y, Xmax, Ymax, anorm, bnorm):
    """(:89-107) on X [b][n], Y [b][m], Xmax [b][n], Ymax [b][mt]: the rollback decision in longdouble with its
    margins from 0.6, the outputs as the f64 restatement x * (bnorm / anorm) (zero tail of Y after a rollback)."""
    X, Y, Xm, Ym = (np.asarray(v, np.complex128) for v in (X, Y, Xmax, Ymax))
    qlast, bnorm = np.asarray(qlast, np.float64), np.asarray(bnorm, np.float64)
    b, m, mt = X.shape[0], Y.shape[1], Ym.shape[1]
    x, x0 = cx(X), cx(Xm)
    re = np.sum(x0[..., 0] * x[..., 0] + x0[..., 1] * x[..., 1], axis=1)
    im = np.sum(x0[..., 0] * x[..., 1] - x0[..., 1] * x[..., 0], axis=1)
    sim = np.sqrt(re * re + im * im) / np.sqrt(np.sum(x0 * x0, axis=(1, 2))) / np.sqrt(np.sum(x * x, axis=(1, 2)))
    roll = (qlast > 0.6) & (sim < LD(0.6))
    s = bnorm / np.float64(np.asarray(anorm).ravel()[0])
    Xo = np.where(roll[:, None], Xm, X) * s[:, None]
    Ypad = np.zeros((b, m), np.complex128)
    Ypad[:, :mt] = Ym
    Yo = np.where(roll[:, None], Ypad, Y) * s[:, None]
    Yo[roll, mt:] = 0
    return Xo, Yo, roll, np.abs((qlast - 0.6) / 0.6), np.abs(np.asarray((sim - LD(0.6)) / LD(0.6), np.float64))


def finalize_f64(opt_obj, optsrc, optysrc, optX, optY, Xcur, Ycur, nc, Zb1=None, Zb2=None, Yb1=None, Yb2=None):
    """(:384-385) with the deferred-copy buffers: returns (Xo [b][nc][n], Yo [b][nc][m], have)."""
    have = np.asarray(opt_obj) < np.inf
    b = len(have)
    Xo = np.empty((b, nc) + np.shape(optX)[2:], np.complex128)
    Yo = np.empty((b, nc) + np.shape(optY)[2:], np.complex128)
    for i in range(b):
        sx = Zb1 if (optsrc[i] == 1 and Zb1 is not None) else Zb2 if (optsrc[i] == 2 and Zb2 is not None) else optX
        sy = Yb1 if (optysrc[i] == 1 and Yb1 is not None) else Yb2 if (optysrc[i] == 2 and Yb2 is not None) else optY
        Xo[i] = np.asarray(sx)[i] if have[i] else np.asarray(Xcur)[i, :nc]
        Yo[i] = np.asarray(sy)[i] if have[i] else np.asarray(Ycur)[i, :nc]
    return Xo, Yo, have


# ---------------------------------------------------------------- part_geinv / part_gfix
def _cmat(x):
    return np.asarray(x, np.complex128).astype(np.clongdouble)


def geinv_ref(Gee):
    """Longdouble inverse of a complex matrix: Gauss-Jordan with partial pivoting, then Newton steps
    X <- X + X (I - G X).  Returns (X, max |G X - I|)."""
    G = _cmat(Gee)
    te = G.shape[0]
    if te == 0:
        return G.copy(), 0.0
    aug = np.concatenate([G, np.eye(te, dtype=np.clongdouble)], axis=1)
    for k in range(te):
        p = k + int(np.argmax(np.abs(aug[k:, k])))
        if p != k:
            aug[[k, p]] = aug[[p, k]]
        aug[k] = aug[k] / aug[k, k]
        f = aug[:, k].copy()
        f[k] = 0
        aug -= f[:, None] * aug[k][None, :]
    X = aug[:, te:]
    eye = np.eye(te, dtype=np.clongdouble)
    for _ in range(3):
        X = X + X @ (eye - G @ X)
    return X, float(np.max(np.abs(G @ X - eye)))


def gj_f64(Gee):
    """The kernel's in-place Gauss-Jordan (no pivoting, the same elimination order) in numpy f64."""
    H = np.array(Gee, np.complex128)
    te = H.shape[0]
    for k in range(te):
        p = H[k, k]
        pr2 = p.real * p.real + p.imag * p.imag
        pinv = complex(p.real / pr2, -p.imag / pr2)
        colk, rowk = H[:, k].copy(), H[k, :].copy()
        upd = H - np.outer(colk * pinv, rowk)
        upd[k, :] = pinv * rowk
        upd[:, k] = -(colk * pinv)
        upd[k, k] = pinv
        H = upd
    return H


def geinv_tol(Gee, X):
    """te u kappa_2(G_ee) ||X||_2: the unit of the inverse's bound (on max |X^ - X|)."""
    te = Gee.shape[0]
    sv = np.linalg.svd(np.asarray(Gee, np.complex128), compute_uv=False)
    return te * U * float(sv[0] / sv[-1]) * float(np.linalg.norm(np.asarray(X, np.complex128), 2))


def gfix_ref(G, geinv, u, rows, mt):
    """g_t = u_t - sum_e conj(G[e][t]) d_e, d = geinv u_e, 0 on the test rows; per realisation.  G [m][m], geinv
    [b][te][te] (any complex type), u [b][r][m], rows [b][m].  Returns (value, tol) with the (re, im) axis."""
    Gl = _cmat(G)
    u = np.asarray(u, np.complex128)
    b, r, m = u.shape
    te = m - mt
    val = np.zeros((b, r, m), np.clongdouble)
    tol = np.zeros((b, r, m), LD)
    for i in range(b):
        tr, tst = rows[i][:mt], rows[i][mt:]
        ul = _cmat(u[i])                                         # [r][m]
        gi = np.asarray(geinv[i]).astype(np.clongdouble).reshape(te, te)
        ue = ul[:, tst]                                          # [r][te]
        d = ue @ gi.T
        e_d = gam(2 * te + 2) * (np.abs(ue) @ np.abs(gi).T)
        Gc = np.conj(Gl[tst, :]).T                               # [m][te]: conj(G[e][t])
        corr = d @ Gc.T                                          # [r][m]
        e_corr = gam(2 * te + 2) * (np.abs(d) @ np.abs(Gc).T) + e_d @ np.abs(Gc).T
        out = ul - corr
        val[i][:, tr] = out[:, tr]
        tol[i][:, tr] = (e_corr + U * np.abs(out))[:, tr]
    v = np.stack([val.real, val.imag], axis=-1)
    return v, np.broadcast_to(tol[..., None], v.shape)


def g_of(A):
    """G = (I + A A^H)^-1 in longdouble (returned as clongdouble), kappa_2(I + K)."""
    Al = _cmat(A)
    m = Al.shape[0]
    Bm = np.eye(m, dtype=np.clongdouble) + Al @ np.conj(Al).T
    G, res = geinv_ref(Bm)
    assert res <= 1e-15 * float(np.max(np.abs(G))) * m + 1e-17, res
    sv = np.linalg.svd(Bm.astype(np.complex128), compute_uv=False)
    return G, float(sv[0] / sv[-1])


def schur_direct(A, T, rows, mt):
    """(I + K_t)^-1 T_t on the train rows (in m-space, 0 on the test rows), K_t = A_t A_t^H; T [r][m]."""
    Al = _cmat(A)
    tr = rows[:mt]
    At = Al[tr]
    Bt = np.eye(mt, dtype=np.clongdouble) + At @ np.conj(At).T
    Xi, _ = geinv_ref(Bt)
    out = np.zeros(T.shape, np.clongdouble)
    out[:, tr] = _cmat(T)[:, tr] @ Xi.T
    return out


def schur_tol(kappa, m, te, T, rows, mt):
    """The identity's bound on ||g - g*||_2 per column (module docstring)."""
    T = np.asarray(T, np.complex128)
    nt = np.linalg.norm(T[:, rows[:mt]], axis=1)
    return U * kappa * (4 * math.sqrt(m) * nt + 4 * te * np.linalg.norm(T, axis=1))


def partition(m, mt, batch, seed):
    """Per-realisation random partitions: rows [b][m] (train rows in sampled order, then the test rows ascending)
    and mask [b][m]."""
    rng = np.random.default_rng(seed)
    rows = np.empty((batch, m), np.int32)
    mask = np.zeros((batch, m), np.uint8)
    for i in range(batch):
        p = rng.permutation(m)
        rows[i, :mt] = p[:mt]
        rows[i, mt:] = np.sort(p[mt:])
        mask[i, p[:mt]] = 1
    return rows, mask


def codebook(m, n, seed):
    """A phase-code codebook (entries in {+-1, +-j} / sqrt(n)), as synth.codebook draws them."""
    rng = np.random.default_rng(seed)
    return (1j ** rng.integers(0, 4, (m, n))) / math.sqrt(n)


def gaussian(m, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))) / math.sqrt(2 * n)


# (kind, m, n, te, r, batch): te crosses the LDS / streamed boundary (48 | 49) and the 64 KiB default (64 | 65), r the
# 8-column chunks
GEINV_CASES = [("code", 100, 64, 0, 1, 3), ("code", 100, 64, 1, 8, 3), ("gauss", 128, 48, 13, 9, 17),
               ("code", 128, 256, 48, 20, 3), ("gauss", 300, 64, 49, 1, 3), ("code", 300, 256, 64, 9, 1),
               ("gauss", 128, 96, 65, 8, 3), ("code", 300, 128, 96, 20, 3), ("gauss", 100, 32, 96, 9, 3)]


@functools.lru_cache(maxsize=None)
def geinv_case(idx):
    """Inputs and references of GEINV_CASES[idx] (computed once per process): dict with G (f64-rounded), kappa,
    rows, mask, Xref [b][te][te] (clongdouble), res (the reference's own residuals), unit (the bound's unit)."""
    kind, m, n, te, r, batch = GEINV_CASES[idx]
    A = codebook(m, n, 100 + idx) if kind == "code" else gaussian(m, n, 100 + idx)
    Gl, kappa = g_of(A)
    G = Gl.astype(np.complex128)
    rows, mask = partition(m, m - te, batch, 200 + idx)
    Xref = np.zeros((batch, te, te), np.clongdouble)
    res, unit = np.zeros(batch), np.zeros(batch)
    for i in range(batch):
        Gee = G[np.ix_(rows[i][m - te:], rows[i][m - te:])]
        Xref[i], res[i] = geinv_ref(Gee)
        unit[i] = geinv_tol(Gee, Xref[i]) if te else 0.0
    rng = np.random.default_rng(300 + idx)
    T = rng.standard_normal((batch, r, m)) + 1j * rng.standard_normal((batch, r, m))
    return dict(A=A, G=G, kappa=kappa, rows=rows, mask=mask, Xref=Xref, res=res, unit=unit, T=T, m=m, mt=m - te, te=te,
                r=r, batch=batch)


# ---------------------------------------------------------------- gram_rotate (:263-264)
def gram_exact(X):
    """H = X^H X of X [r][n] (column j of the n x r iterate is X[j]) as an mp matrix, formed in Python integers."""
    X = np.asarray(X, np.complex128)
    r = X.shape[0]
    re, im, s = ZR._int_matrix(X)                        # rows: the columns x_j
    cre = [[v for v in row] for row in re]
    cim = [[-v for v in row] for row in im]              # conj(x_i) . x_j
    hr, hi = ZR._int_matmul(cre, cim, re, im)
    sc = mp.mpf(2) ** (2 * s)
    H = mp.matrix(r, r)
    for i in range(r):
        for j in range(r):
            H[i, j] = mp.mpc(hr[i][j], hi[i][j]) * sc
    return H


def gram_ref(X):
    """Eigenpairs of the exact Gram matrix at DPS digits, ascending: dict(lam [r] f64-able mp, V [r][r] clongdouble
    (column k = v_k), normH, relgap [r] (distance to the nearest other eigenvalue over ||H||))."""
    with mp.workdps(DPS):
        H = gram_exact(X)
        lam, V = mp.eigh(H)
        r = H.rows
        lam = [lam[i] for i in range(r)]
        order = sorted(range(r), key=lambda i: lam[i])
        lam_s = [lam[i] for i in order]
        Vn = np.empty((r, r), np.clongdouble)
        for c, i in enumerate(order):
            for k in range(r):
                Vn[k, c] = LD(float(mp.re(V[k, i]))) + LD(float(mp.re(V[k, i]) - float(mp.re(V[k, i])))) + 1j * (
                    LD(float(mp.im(V[k, i]))) + LD(float(mp.im(V[k, i]) - float(mp.im(V[k, i])))))
        top = max(abs(lam_s[-1]), mp.mpf(0))
        lam_f = np.array([LD(float(v)) + LD(float(v - float(v))) for v in lam_s], LD)
        relgap = np.full(r, math.inf)
        for k in range(r):
            for j in range(r):
                if j != k and top > 0:
                    relgap[k] = min(relgap[k], float(abs(lam_s[k] - lam_s[j]) / top))
    return dict(lam=lam_f, V=Vn, normH=float(top), relgap=relgap)


def gram_stats(X, Xout, ref, rank=None):
    """The four figures of the module docstring for one realisation (X, Xout [r][n]); rank: the input's rank when it
    is deficient (the r - rank smallest eigenvalues are null).  Returns dict(a, orth-free; b, c, d in their units,
    asc: the ascending-order check, null: largest null-column norm over sqrt(u) ||X||_2)."""
    Xl, Yl = _cmat(X).T, _cmat(Xout).T                           # n x r
    r = Xl.shape[1]
    nx2 = float(np.sum(np.abs(Xl) ** 2))
    a = float(np.sqrt(np.sum(np.abs(Yl @ np.conj(Yl).T - Xl @ np.conj(Xl).T) ** 2))) / (U * nx2) if nx2 else 0.0
    O = np.conj(Yl).T @ Yl
    dn = np.real(np.diag(O))
    lam, normH = ref["lam"], ref["normH"]
    x2 = math.sqrt(normH)                                        # ||X||_2
    first = 0 if rank is None else r - rank
    live = range(first, r)
    kap = float(lam[-1] / lam[first]) if normH > 0 else 1.0
    bfig = 0.0
    for i in live:
        for j in live:
            if i != j:
                bfig = max(bfig, float(np.abs(O[i, j]) / np.sqrt(dn[i] * dn[j])) / (U * kap))
    null = max((float(np.sqrt(dn[k])) / (math.sqrt(U) * x2) for k in range(first)), default=0.0)
    cfig = dfig = 0.0
    asc = True
    if rank is None:
        for k in range(r):
            if ref["relgap"][k] < GAP:
                continue
            cfig = max(cfig, float(np.abs(dn[k] - lam[k])) / (U * normH))
            t = Xl @ ref["V"][:, k]
            ph = np.vdot(t, Yl[:, k])
            ph = ph / np.abs(ph) if np.abs(ph) > 0 else 1
            gapk = min(ref["relgap"][k], 1.0) * normH            # (r = 1: no other eigenvalue)
            dfig = max(dfig, float(np.sqrt(np.sum(np.abs(Yl[:, k] - ph * t) ** 2))) / (U * normH / gapk * x2))
            if k + 1 < r and ref["relgap"][k + 1] >= GAP and not dn[k] < dn[k + 1]:
                asc = False
    return dict(a=a, b=bfig, c=cfig, d=dfig, asc=asc, null=null)


def gram_tol_a(r):
    return 2 * (2 * 32 + 2) * math.sqrt(r) + GRAM_MULT * GRAM_ORACLE["orth"] * r


def gram_oracle(X):
    """The f64 oracle of the rotation: numpy.linalg.eigh on fl(X^H X), X V (X [r][n])."""
    Xc = np.asarray(X, np.complex128).T
    w, V = np.linalg.eigh(Xc.conj().T @ Xc)
    return np.ascontiguousarray((Xc @ V).T), V


def gram_input(kind, n, r, seed):
    """One realisation's X [r][n].  full: separated spectrum (singular values 1 .. r through random unitary factors);
    rank3: rank 3 < r; hadamard: X = Hn[:, :r] diag(s) Hr^T, integer entries, X^H X = n Hr diag(s^2) Hr^T with two
    equal s (n, r powers of two).  Returns (X, rank or None, exact eigenvalues ascending or None)."""
    rng = np.random.default_rng(seed)
    if kind == "hadamard":
        s = np.arange(1, r + 1, dtype=np.int64)
        if r >= 2:
            s[-1] = s[-2]                                        # two equal eigenvalues (the largest)
        X = ZR.hadamard(n)[:, :r] @ np.diag(s) @ ZR.hadamard(r).T
        lam = np.sort((n * r * s * s).astype(np.float64))
        return np.ascontiguousarray(X.T.astype(np.complex128)), None, lam
    k = min(n, r) if kind == "full" else min(3, n, r)
    Ql, _ = np.linalg.qr(rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k)))
    Qr, _ = np.linalg.qr(rng.standard_normal((r, k)) + 1j * rng.standard_normal((r, k)))
    sv = np.arange(1, k + 1, dtype=np.float64)
    X = (Ql * sv) @ Qr.conj().T                                  # n x r
    return np.ascontiguousarray(X.T), (None if kind == "full" and k == r else k), None


# (kind, n, r, batch): every n and r of the issue; "full" needs n >= r for full rank
GRAM_CASES = [("full", 1, 1, 3), ("full", 31, 2, 17), ("full", 32, 19, 3), ("full", 33, 20, 1), ("full", 256, 31, 3),
              ("full", 257, 32, 3), ("rank3", 31, 19, 3), ("rank3", 257, 32, 1), ("rank3", 33, 20, 17),
              ("rank3", 1, 2, 3), ("hadamard", 32, 2, 3), ("hadamard", 256, 32, 1), ("hadamard", 32, 16, 3)]


@functools.lru_cache(maxsize=None)
def gram_case(idx):
    """Inputs of GRAM_CASES[idx]: X [b][r][n], rank, and the mp references of the distinct realisations (the batch
    cycles through at most three distinct inputs, so a reference is computed once per distinct input)."""
    kind, n, r, batch = GRAM_CASES[idx]
    distinct = min(batch, 3)
    ins = [gram_input(kind, n, r, 1000 * idx + d) for d in range(distinct)]
    refs = [gram_ref(x) for x, _, _ in ins]
    X = np.stack([ins[i % distinct][0] for i in range(batch)])
    if kind == "rank3" and n == 1:
        rank = 1
    else:
        rank = ins[0][1]
    return dict(X=X, rank=rank, refs=[refs[i % distinct] for i in range(batch)], lam_exact=ins[0][2], kind=kind, n=n,
                r=r, batch=batch)


# ---------------------------------------------------------------- inputs of the init / Y-step suite
# (m, n, r, batch): every m, n, r of the issue once
YCASES = [(1, 1, 1, 17), (5, 31, 2, 3), (255, 257, 19, 1), (257, 1, 20, 3), (300, 31, 32, 17)]


def ystep_inputs(m, r, batch, seed, mask=False):
    """S, g, M, B, Yold, mu of a Y-step.  Row 2 (m >= 5) is a zero row in all columns (S == g, M = 0), row 3 in
    column 0 only; with batch 17 the last realisation repeats the first (position invariance)."""
    rng = np.random.default_rng(seed)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)   # noqa: E731
    S, g, M, Yold = c(batch, r, m), c(batch, r, m), 0.1 * c(batch, r, m), c(batch, r, m)
    B = np.abs(rng.standard_normal((batch, m))) + 0.1
    mu = rng.uniform(0.5, 2.0, batch)
    if m >= 5:
        g[:, :, 2] = S[:, :, 2]
        M[:, :, 2] = 0
        g[:, 0, 3] = S[:, 0, 3]
        M[:, 0, 3] = 0
    mk = None
    if mask:
        mk = (rng.uniform(size=(batch, m)) < 0.8).astype(np.uint8)
        mk[:, 0] = 1
        if m >= 5:
            mk[:, 2:4] = 1
    if batch == 17:
        for v in (S, g, M, Yold, B, mu) + (() if mk is None else (mk,)):
            v[16] = v[0]
    return dict(S=S, g=g, M=M, B=B, Y=Yold, mu=mu, mask=mk)


def init_inputs(m, n, r, batch, seed, mask=False):
    """X0, P0, B of an init; rows 2 and 3 as in ``ystep_inputs`` (P0 = 0 there)."""
    rng = np.random.default_rng(seed)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)   # noqa: E731
    X0, P0 = c(batch, r, n), c(batch, r, m)
    B = np.abs(rng.standard_normal((batch, m))) + 0.1
    if m >= 5:
        P0[:, :, 2] = 0
        P0[:, 0, 3] = 0
    mk = None
    if mask:
        mk = (rng.uniform(size=(batch, m)) < 0.8).astype(np.uint8)
        mk[:, 0] = 1
        if m >= 5:
            mk[:, 2:4] = 1
    if batch == 17:
        for v in (X0, P0, B) + (() if mk is None else (mk,)):
            v[16] = v[0]
    return dict(X=X0, P0=P0, B=B, mask=mk)


def column_specials(m, r, seed):
    """Column-mode Y-step inputs (batch 3) for the argmin's edges: realisation 0 has a NaN objective in column 1
    (skipped), realisation 1 in column 0 (the first finite column wins unless a later one is smaller), realisation
    2 has columns 1 and 2 equal to the otherwise best column arrangement: an exact tie, the first index wins."""
    d = ystep_inputs(m, r, 3, seed)
    S = d["S"]
    S[0, 1, 0] = np.nan
    S[1, 0, m - 1] = np.nan
    # realisation 2: make column 1 the clear minimiser (A X close to B in modulus), then duplicate it into column 2
    ph = np.exp(1j * np.linspace(0, 3, m))
    S[2, 1] = d["g"][2, 1] + d["B"][2] * ph * (1 + 1e-3)
    for k in ("S", "g", "M", "Y"):
        d[k][2, 2] = d[k][2, 1]
    return d


def exact_quality_inputs():
    """|a_i x| = b_i exactly on integer data (a_i x in {3 + 4j, 5 + 12j, 8 - 15j, ...}): quality is exactly 1."""
    trip = [(3, 4, 5), (5, 12, 13), (8, -15, 17), (-7, 24, 25), (20, 21, 29)]
    n, b = 6, 3
    X = np.zeros((b, n), np.complex128)
    X[:, 0] = [1, 1j, -1]
    X[:, 1] = [2, 2, 2j]
    A = np.zeros((len(trip), n), np.complex128)
    B = np.zeros((b, len(trip)))
    for i, (p, q, h) in enumerate(trip):
        A[i, 0] = p + 1j * q                                     # a_i x = (p + jq) x_0 + 0: |.| = h |x_0|
        A[i, 2:] = i + 1                                         # times x = 0
        B[:, i] = h
    return A, X, B


def finish_cases():
    """qlast, X, Y, Xmax, Ymax, anorm, bnorm at n = 37, m = 21, mt = 17, batch 6: rollback (q > 0.6, sim < 0.6), no
    rollback by similarity, no rollback by quality, qlast == 0.6 exactly with a small similarity (no rollback), and
    two more with the roles mixed."""
    rng = np.random.default_rng(9)
    n, m, mt, b = 37, 21, 17, 6
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)   # noqa: E731
    Xm, Y, Ym = c(b, n), c(b, m), c(b, mt)
    X = c(b, n)
    for i in (1, 4):
        X[i] = Xm[i] * (0.7 - 0.2j) + 0.05 * c(n)                # similar: sim about 1
    qlast = np.array([0.9, 0.9, 0.3, 0.6, 0.61, 0.59])
    return dict(q=qlast, X=X, Y=Y, Xmax=Xm, Ymax=Ym, anorm=np.array([1.7]), bnorm=rng.uniform(0.5, 2, b))
