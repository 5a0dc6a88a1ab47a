"""Numpy restatement (float64 / complex128) of the Bayesian A-optimal row exchange, bayesAopt_complex.m:105-254 as
Bayes_Beam.m:12 calls it: A = I, K = kdiag I, no fixed rows.  The oracle of tests/test_aopt_ref.py and
tests/test_gpu_aopt.py, and the CPU baseline of tools/bench_aopt.py.

Candidates are the rows f_i of F [P][n], x_i = f_i^H.  State of a design: Minv = (X^H X + K)^-1,
g_i = x_i^H Minv x_i, t_i = ||Minv x_i||^2, Acrit = trace(Minv), rowlist.  The reference's NinvF (:233) is
formed there and never read; it is not formed here.

Beside the selection the restatement records, for every step, the relative gap between the two smallest
exchange values ``ad`` (entries that equal the minimum exactly -- duplicated candidate rows -- do not count as
the second one), and for every step on an assigned row |a - acutoff|: the margins a second implementation
with another summation order has to stay within to take the same decisions.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

ACUTOFF = -float(np.sqrt(np.finfo(np.float64).eps))
ST_SINGULAR = 65536   # ACE_ST_AOPT_SINGULAR


@dataclass
class AoptRef:
    rowlist: np.ndarray      # [nrows] int32 candidate index per design row
    acrit: np.ndarray        # [2]: trace(Minv) at the start, tracked value at the end
    iters: int
    switches: int
    status: int
    Minv: np.ndarray         # [n][n] tracked inverse
    gaps: list = field(default_factory=list)       # per step: (ad_2nd - ad_min) / max(|ad_min|, |ad_2nd|)
    cut_margin: list = field(default_factory=list)  # per step on an assigned row: |a - acutoff|
    acrit_pass: list = field(default_factory=list)  # tracked Acrit after every pass


def _dots(F, u, blas):
    """sum_k F[i][k] u[k] for every row i.  Without ``blas`` each row is summed on its own by the same
    procedure, so equal rows give equal bits wherever they stand (a BLAS kernel may block rows)."""
    return F @ u if blas else (F * u[None, :]).sum(axis=1)


def brute_minv(F, rows, kdiag=1.0):
    X = np.asarray(F)[np.asarray(rows, dtype=np.int64)]
    return np.linalg.inv(X.conj().T @ X + kdiag * np.eye(F.shape[1]))


def aopt_select(F, nrows, init, kdiag=1.0, maxiter=5, acutoff=ACUTOFF, blas=False) -> AoptRef:
    F = np.ascontiguousarray(np.asarray(F, dtype=np.complex128))
    P, n = F.shape
    nrows = int(nrows)
    cur = np.asarray(init, dtype=np.int64).reshape(-1)[:nrows].copy()
    assert cur.size == nrows and cur.min() >= 0 and cur.max() < P
    Minv = brute_minv(F, cur, kdiag)
    MinvF = Minv @ F.conj().T                                  # column i: Minv x_i          (:181)
    g = np.real((F.T * MinvF).sum(axis=0))                     # x_i^H Minv x_i            (:185)
    t = (np.abs(MinvF) ** 2).sum(axis=0)                       # ||Minv x_i||^2            (:182)
    acrit0 = acrit = float(np.real(np.trace(Minv)))
    rowlist = np.full(nrows, -1, np.int32)
    res = AoptRef(rowlist, np.zeros(2), 0, 0, 0, Minv)
    it, made = 0, True
    while made and it < maxiter and not res.status:
        made = False
        it += 1
        for r in range(nrows):
            x = F[cur[r]].conj()
            u = Minv @ x
            den = 1.0 - float(np.real(np.vdot(x, u)))
            if not (np.isfinite(den) and den > 0.0):
                res.status |= ST_SINGULAR
                break
            w = 1.0 / den
            v = Minv @ u
            beta = float(np.real(np.vdot(u, u)))
            p = _dots(F, u, blas).conj()                       # u^H x_i
            q = _dots(F, v, blas).conj()
            ap2 = p.real * p.real + p.imag * p.imag
            gn = g + w * ap2
            W = 1.0 / (1.0 + gn)
            tn = t + 2.0 * w * (q.real * p.real + q.imag * p.imag) + beta * w * w * ap2
            ad = w * beta - W * tn
            j = int(np.argmin(ad))                             # first index of the minimum
            a = float(ad[j])
            rest = ad[ad != a]
            if rest.size:
                b = float(rest.min())
                res.gaps.append((b - a) / max(abs(a), abs(b)))
            if rowlist[r] >= 0:
                res.cut_margin.append(abs(a - acutoff))
            if a < acutoff or rowlist[r] < 0:
                made = True
                acrit += a
                res.switches += 1
                rowlist[r] = j
                cur[r] = j
                Ninv = Minv + w * np.outer(u, u.conj())
                up = Ninv @ F[j].conj()
                wp = float(W[j])
                vp = Ninv @ up
                betap = float(np.real(np.vdot(up, up)))
                pp = _dots(F, up, blas).conj()
                qp = _dots(F, vp, blas).conj()
                app2 = pp.real * pp.real + pp.imag * pp.imag
                Minv = Ninv - wp * np.outer(up, up.conj())
                g = gn - wp * app2
                t = tn - 2.0 * wp * (qp.real * pp.real + qp.imag * pp.imag) + betap * wp * wp * app2
        res.acrit_pass.append(acrit)
    res.acrit[:] = (acrit0, acrit)
    res.iters = it
    res.Minv = Minv
    return res
