"""Extended-precision reference, known-answer inputs and derived tolerances for the Z-step of the ADMM
iteration (tests/test_gpu_zprox.py; self-tested on the CPU by tests/test_zprox_ref.py).

    Z' = ArgMinZ(X + N/mu)        N' = N + mu (X - Z')        iteration control (:344-381)

(a) General reference
---------------------
``argmin_z_ref`` transcribes ArgMinZ (inferLowRankV4_multi.m:424-484) line by line at 40 digits (mpmath):
E = X + N/mu exactly, H = E E^H exactly (every operand is an f64, so the Gram matrix is an exact dyadic
rational: it is formed in Python integers), ``mp.eigh``, the clamp max(0, .), MATLAB's stable descending sort,
the sequential in-place profile loop (vr and v are re-read from the spectrum the earlier entries scaled),
sqrt(scale) and the ``any(scale < 1)`` shortcut.  Z = U diag(sqrt(scale)) U^H E is again an integer product (U
diag U^H rounded to 2^-150).  Z is returned as an unevaluated sum hi + lo of two f64
arrays (N' as a longdouble array), so a comparison does not start from a reference rounded to f64.  ``iter_control_ref`` transcribes the
sums and the control of the iteration (:344-351, :364-381) the same way.

(b) Known-answer inputs
-----------------------
``known_answer`` builds E = D1 P1 Hd diag(s) Hd'^T P2 D2 / 2^k from Sylvester-Hadamard matrices Hd (tx x tx) and
Hd' (rx x rx), permutations, diagonals in {+-1, +-j} and integer s.  Every entry of E is an integer over 2^k,
exact in f64.  E E^H = (tx rx / 4^k) sum_i s_i^2 u_i u_i^H with u_i = D1 P1 Hd[:, i] / sqrt(tx): the eigenvectors
are known columns and the eigenvalues exact rationals, so the profile loop runs in ``fractions.Fraction`` and Z
needs one square root per group and no eigensolver.

(c) Tolerance
-------------
Write Z = f(H) E with f(lambda_i) = sqrt(c_i), c_i the accumulated scale of eigenvalue i.  An eigensolver with
backward error eta ||H|| returns the exact decomposition of H + D, ||D|| <= eta ||H||.  To first order
(Daleckii-Krein: the Frechet derivative of a spectral function is the Hadamard product with the divided
differences (f_i - f_j) / (lambda_i - lambda_j), which vanish inside a group of equal f)

    || Z - Z* ||_F  <=  eta kappa || E ||_F,        kappa = kappa_vec + kappa_scale + 1,
    kappa_vec   = ||H||_2 max over pairs with c_i != c_j of |sqrt c_i - sqrt c_j| / |lambda_i - lambda_j|,
    kappa_scale = sum over fired entries (r, f) of  1/2 ||H||_2 ( r / vr + (tx - r) / (v - vr) ):

a fired entry's scale is vr / (v - vr) (1/f - 1) with vr the sum of r and v - vr of tx - r eigenvalues, each
moved by at most eta ||H|| (Weyl), and the factor applied is its square root (the 1/2); entries clamped at
scale = 1 contribute nothing.  The 1 covers forming E, the final product and the output rounding.  The
tolerance of a case is TOL_MULT u kappa (u = 2^-53) on || Z - Z* ||_F / || E ||_F.  TOL_MULT is not chosen
by looking at the kernels: tests/test_zprox_ref.py measures the largest ratio err / (u kappa) that the f64
oracle ``ace_oracle.argmin_z_lowrank`` (LAPACK's zheevd) reaches against this reference over the inputs of the
GPU suite, asserts it stays below ORACLE_RATIO, and the kernels get 8 x ORACLE_RATIO (Jacobi and
Householder + twisted factorisation differ from LAPACK's solver by a modest polynomial factor).

The reference also reports which entries fired, the smallest relative distance of a ``vr < v f`` decision (and
of the min(1, .) clamp) from equality, and the smallest relative eigenvalue gap (over ||H||) across a boundary
where the scale changes: the GPU suite compares Z only where the decisions are at least 1e-6 and the gaps at
least 1e-3 away, as shown on the reference alone.
"""
import functools
import math
from dataclasses import dataclass, field
from fractions import Fraction

import mpmath as mp
import numpy as np

import ace_oracle as O

U = 2.0 ** -53
DPS = 40
WBITS = 150          # U diag(sqrt(scale)) U^H is rounded to multiples of 2^-WBITS before the integer product
# largest err / (u kappa) of the f64 oracle against the reference over the suite's inputs, rounded up
# (measured 1.105 at 8x8-b65[64]; tests/test_zprox_ref.py::test_oracle_inside_tolerance prints it), and the
# kernels' multiplier
ORACLE_RATIO = 1.11
TOL_MULT = 8.0 * ORACLE_RATIO


# ---------------------------------------------------------------- layout
def to_E(x, tx):
    """[r][n] iterate (each column a column-major tx x rx matrix) -> E = reshape(., tx, []) (tx x r rx)."""
    x = np.asarray(x)
    return np.ascontiguousarray(x.reshape(-1, tx).T)


def from_E(E, r):
    """Inverse of ``to_E``: tx x (r rx) -> [r][n]."""
    E = np.asarray(E)
    return np.ascontiguousarray(E.T.reshape(r, -1))


# ---------------------------------------------------------------- exact integer products
def _dyadic(x):
    """f64 -> (integer mantissa, exponent) with x = mant 2^exp exactly."""
    if x == 0.0:
        return 0, 0
    mnt, e = math.frexp(x)
    return int(mnt * (1 << 53)), e - 53


def _int_matrix(A, dA=None):
    """Complex f64 matrix A (+ dA) -> (re, im) nested lists of Python ints and a shift s, A + dA = (re + j im) 2^s."""
    A = np.ascontiguousarray(np.asarray(A, np.complex128))
    mats = [A] if dA is None else [A, np.ascontiguousarray(np.asarray(dA, np.complex128))]
    for M in mats:
        if not np.all(np.isfinite(M.view(np.float64))):
            raise ValueError("non-finite input")
    parts = [[[(_dyadic(float(v.real)), _dyadic(float(v.imag))) for v in row] for row in M] for M in mats]
    exps = [e for P in parts for row in P for pr in row for (mnt, e) in pr if mnt]
    s = min(exps) if exps else 0
    rows, cols = A.shape
    re = [[sum(P[i][j][0][0] << (P[i][j][0][1] - s) for P in parts if P[i][j][0][0]) for j in range(cols)]
          for i in range(rows)]
    im = [[sum(P[i][j][1][0] << (P[i][j][1][1] - s) for P in parts if P[i][j][1][0]) for j in range(cols)]
          for i in range(rows)]
    return re, im, s


def _mp_int_matrix(W, bits):
    """mp matrix -> (re, im) integer lists with W ~ (re + j im) 2^-bits (rounded to nearest)."""
    sc = mp.mpf(2) ** bits
    re = [[int(mp.nint(mp.re(W[i, j]) * sc)) for j in range(W.cols)] for i in range(W.rows)]
    im = [[int(mp.nint(mp.im(W[i, j]) * sc)) for j in range(W.cols)] for i in range(W.rows)]
    return re, im


def _int_matmul(ar, ai, br, bi):
    """(ar + j ai) (br + j bi) over Python ints; b given as its transpose's rows (list of columns)."""
    outr, outi = [], []
    for xr, xi in zip(ar, ai):
        rr, ri = [], []
        for yr, yi in zip(br, bi):
            sr = si = 0
            for p, q, u_, v_ in zip(xr, xi, yr, yi):
                sr += p * u_ - q * v_
                si += p * v_ + q * u_
            rr.append(sr)
            ri.append(si)
        outr.append(rr)
        outi.append(ri)
    return outr, outi


def _hilo(num, shift):
    """Integer num 2^shift -> (hi, lo) f64 with hi + lo = the value to about 2^-106."""
    f = Fraction(num) * (Fraction(2) ** shift)
    hi = float(f)
    return hi, float(f - Fraction(hi))


def _hilo_matrix(re, im, shift):
    hi = np.empty((len(re), len(re[0])), np.complex128)
    lo = np.empty_like(hi)
    for i, (rr, ri) in enumerate(zip(re, im)):
        for j, (a, b) in enumerate(zip(rr, ri)):
            ah, al = _hilo(a, shift)
            bh, bl = _hilo(b, shift)
            hi[i, j] = complex(ah, bh)
            lo[i, j] = complex(al, bl)
    return hi, lo


# ---------------------------------------------------------------- (a) the general reference
@dataclass
class ZRef:
    """Reference Z-step of one realisation.  Z = Z_hi + Z_lo (tx x cols); lam: sorted clamped spectrum of E E^H;
    scale: accumulated c_i in that order; fired: per profile entry; margin: smallest relative distance of a
    decision from equality; gap: smallest relative eigenvalue gap across a scale-changing boundary."""
    E: np.ndarray
    Z_hi: np.ndarray
    Z_lo: np.ndarray
    lam: list
    scale: list
    fired: list
    any_fired: bool
    kappa_vec: float
    kappa_scale: float
    margin: float
    gap: float
    normE: float
    W: object = field(default=None, repr=False)   # U diag(sqrt(scale)) U^H (mp matrix) when a rescaling fired

    @property
    def kappa(self):
        return self.kappa_vec + self.kappa_scale + 1.0

    @property
    def tol(self):
        """Bound on || Z - Z* ||_F / || E ||_F for the kernels."""
        return TOL_MULT * U * self.kappa

    def err(self, Z):
        """|| Z - Z* ||_F / || E ||_F of a computed tx x cols matrix."""
        d = (np.asarray(Z, np.complex128) - self.Z_hi) - self.Z_lo
        return float(np.linalg.norm(d)) / self.normE if self.normE > 0 else float(np.linalg.norm(d))

    def singular_values(self):
        """Singular values of Z*: sqrt(c_i lambda_i), descending."""
        return sorted((math.sqrt(c * l) for c, l in zip(self.scale, self.lam)), reverse=True)


def profile_loop(lam, rl, fl, num=mp.mpf):
    """The sequential in-place loop (:469-480) on a descending spectrum; ``num`` is the number type (mp.mpf or
    Fraction).  Returns (scale per sorted position, fired flags, per fired entry (r, vr, v), margin)."""
    tx = len(lam)
    s2 = list(lam)
    sc = [num(1)] * tx
    fired, info, margin = [], [], math.inf
    for rr, f in zip(rl, fl):
        f = num(f) if num is not Fraction else Fraction(f)   # the f64 value of the literal, as MATLAB holds it
        vr = sum(s2[:rr], num(0))
        v = sum(s2, num(0))
        if v > 0:
            margin = min(margin, abs(float((vr - v * f) / (v * f))))
        if vr < v * f:
            c = vr / (v - vr) * (1 / f - 1)
            margin = min(margin, abs(float(c - 1)))
            if c > 1:
                c = num(1)
            for k in range(rr, tx):
                s2[k] *= c
                sc[k] *= c
            fired.append(True)
            info.append((rr, float(vr), float(v), float(c)))
        else:
            fired.append(False)
    return sc, fired, info, margin


def _kappa(lam, sc, info):
    """kappa_vec, kappa_scale and the boundary gap from the sorted spectrum and the accumulated scales."""
    tx = len(lam)
    top = float(lam[0]) if lam else 0.0
    if top == 0.0:
        return 0.0, 0.0, math.inf
    fs = [math.sqrt(float(c)) for c in sc]
    kv, gap = 0.0, math.inf
    for i in range(tx):
        for j in range(i + 1, tx):
            if sc[i] != sc[j]:
                d = abs(float(lam[i] - lam[j]))
                kv = max(kv, math.inf if d == 0.0 else abs(fs[i] - fs[j]) / d * top)
    for k in range(1, tx):
        if sc[k] != sc[k - 1]:
            gap = min(gap, float(lam[k - 1] - lam[k]) / top)
    ks = 0.0
    for rr, vr, v, c in info:
        if c < 1.0:
            ks += 0.5 * top * (rr / vr + (tx - rr) / (v - vr))
    return kv, ks, gap


def argmin_z_ref(E, rl, fl, dE=None):
    """ArgMinZ (:424-484) of E + dE (tx x cols complex f64 each; dE: the part of X + N/mu that E, its rounding to
    f64, leaves out -- ``exact_E``; None: zero) at DPS digits.  Returns a ZRef."""
    E = np.ascontiguousarray(np.asarray(E, np.complex128))
    tx, cols = E.shape
    with mp.workdps(DPS):
        er, ei, s = _int_matrix(E, dE)
        hr, hi_ = _int_matmul(er, ei, er, [[-v for v in row] for row in ei])   # E E^H: rows of conj(E) on the right
        H = mp.matrix(tx, tx)
        for i in range(tx):
            for j in range(tx):
                H[i, j] = mp.mpc(mp.ldexp(mp.mpf(hr[i][j]), 2 * s), mp.ldexp(mp.mpf(hi_[i][j]), 2 * s))
        w, Uv = mp.eigh(H)                                  # :428, ascending
        lam0 = [max(mp.mpf(0), w[i]) for i in range(tx)]    # :429
        idx = sorted(range(tx), key=lambda i: -lam0[i])     # :430 (stable)
        lam = [lam0[i] for i in idx]
        sc, fired, info, margin = profile_loop(lam, rl, fl)
        kv, ks, gap = _kappa(lam, sc, info)
        normE = float(mp.sqrt(sum(lam0, mp.mpf(0))))
        any_fired = any(c < 1 for c in sc)                  # :482
        W = None
        if any_fired:
            D = mp.matrix(tx, tx)
            for k, i in enumerate(idx):
                D[i, i] = mp.sqrt(sc[k])
            W = Uv * D * Uv.H
            wr, wi = _mp_int_matrix(W, WBITS)
            etr = [list(c) for c in zip(*er)]               # columns of E
            eti = [list(c) for c in zip(*ei)]
            zr, zi = _int_matmul(wr, wi, etr, eti)
            Z_hi, Z_lo = _hilo_matrix(zr, zi, s - WBITS)
        else:
            Z_hi, Z_lo = E.copy(), (np.zeros_like(E) if dE is None else np.asarray(dE, np.complex128).copy())
        return ZRef(E=E, Z_hi=Z_hi, Z_lo=Z_lo, lam=[float(x) for x in lam], scale=[float(c) for c in sc],
                    fired=fired, any_fired=any_fired, kappa_vec=kv, kappa_scale=ks, margin=margin, gap=gap,
                    normE=normE, W=W)


def exact_E(X, N, mu):
    """E = X + N/mu (:424) as the f64 matrix nearest to the exact value (one rounding per component), with the
    residual: returns (E, dE) f64 arrays, E + dE exact to 2^-106.  N = 0: E = X exactly."""
    X = np.asarray(X, np.complex128)
    N = np.asarray(N, np.complex128)
    if not N.any():
        return X.copy(), np.zeros_like(X)
    mu = Fraction(float(mu))
    xf, nf = X.ravel().view(np.float64), N.ravel().view(np.float64)
    e = np.empty_like(xf)
    de = np.empty_like(xf)
    for k in range(xf.size):
        v = Fraction(float(xf[k])) + Fraction(float(nf[k])) / mu
        e[k] = float(v)
        de[k] = float(v - Fraction(e[k]))
    return e.view(np.complex128).reshape(X.shape), de.view(np.complex128).reshape(X.shape)


def xw_ref(Z, N, W, mu):
    """The wmode iterate X = fl(fl(Z - N fl(1/mu)) + W): the rounding sequence every producer of X uses (an fma,
    then an addition), evaluated with exact rationals and rounded where the kernels round."""
    Z, N, W = (np.asarray(a, np.complex128) for a in (Z, N, W))
    if not N.any():
        return Z + W
    imu = Fraction(1.0 / float(mu))
    zf, nf, wf = (a.ravel().view(np.float64) for a in (Z, N, W))
    out = np.empty_like(zf)
    for k in range(zf.size):
        v = float(Fraction(float(zf[k])) - Fraction(float(nf[k])) * imu)
        out[k] = v + wf[k]
    return out.view(np.complex128).reshape(Z.shape)


def n_update_ref(N, mu, X, ref):
    """N' = N + mu (X - Z*) in extended precision (a clongdouble array shaped like X, tx x cols here; its own
    error is a few 2^-64 of |N| + mu |X - Z|, against tolerances of several 2^-53 of the same)."""
    ld = np.clongdouble
    d = (np.asarray(X, np.complex128).astype(ld) - ref.Z_hi.astype(ld)) - ref.Z_lo.astype(ld)
    return np.asarray(N, np.complex128).astype(ld) + np.longdouble(mu) * d


def n_tol(N_new, mu, X, Z_new, ref):
    """Bound on || N' - N'* ||_F: mu times the Z tolerance plus the three roundings of n + mu (x - z)."""
    return mu * ref.tol * ref.normE + 3 * U * (np.linalg.norm(N_new) + 2 * mu * np.linalg.norm(np.asarray(X) - Z_new))


# ---------------------------------------------------------------- the sums and the iteration control
def _norm2(hi, lo=None):
    a = np.asarray(hi, np.complex128).ravel().view(np.float64)
    if lo is None:
        return mp.fsum(mp.mpf(float(v)) ** 2 for v in a)
    b = np.asarray(lo, np.complex128).ravel().view(np.float64)
    return mp.fsum((mp.mpf(float(v)) + mp.mpf(float(w_))) ** 2 for v, w_ in zip(a, b))


def iter_control_ref(X, Z0, ref, *, mu, m, n, r, st, tol_rel, tol_abs, rho, fixed_iters):
    """The bookkeeping of one iteration after the Z-step (:344-351 best objective, :364-370 residuals and
    thresholds, :372 stop test, :379-381 mu update) at DPS digits.  X, Z0: tx x cols f64 (the iterate and the
    previous Z); ref: the ZRef of this step; st: the scalars the Y-step left (obj2, nAX2, nY2, nJM2, dY2, dAtY,
    nAtY) and opt_obj, last_res.  Returns a dict with the results and ``margin``, the smallest relative distance
    of a comparison from equality."""
    with mp.workdps(DPS):
        X = np.asarray(X, np.complex128)
        nX2 = _norm2(X)
        nZ2 = _norm2(ref.Z_hi, ref.Z_lo)
        jn2 = _norm2(X - ref.Z_hi, -ref.Z_lo)      # (X - Z_hi is exact where it matters: Sterbenz or Z = E = X)
        dZ2 = _norm2(ref.Z_hi - np.asarray(Z0, np.complex128), ref.Z_lo)
        g = lambda k: mp.mpf(float(st.get(k, 0.0)))   # noqa: E731
        obj = mp.sqrt(g("obj2"))
        opt_obj = g("opt_obj")
        last_res = g("last_res")
        nAX, nY, nX, nZ = mp.sqrt(g("nAX2")), mp.sqrt(g("nY2")), mp.sqrt(nX2), mp.sqrt(nZ2)
        dAtY2, nAtY2 = max(mp.mpf(0), g("dAtY")), max(mp.mpf(0), g("nAtY"))
        muq = mp.mpf(float(mu))
        res_prim = mp.sqrt(g("nJM2") + jn2)
        res_dual = muq * mp.sqrt(dAtY2 + dZ2)
        res_comb = mp.sqrt(res_prim ** 2 + g("dY2") + dZ2)
        ta, tr = mp.mpf(float(tol_abs)), mp.mpf(float(tol_rel))
        mx1, mx2 = max(nAX, nY), max(nX, nZ)
        t_prim = ta * mp.sqrt((m + n) * r) + tr * mp.sqrt(mx1 ** 2 + mx2 ** 2)
        t_dual = ta * mp.sqrt(n * r * 2) + tr * mp.sqrt(nAtY2 + nZ ** 2)
        t_comb = ta * mp.sqrt((m + n) * r * 2) + tr * mp.sqrt(mx1 ** 2 + mx2 ** 2 + nY ** 2 + nZ ** 2)

        def dist(a, b):
            if mp.isinf(a) or mp.isinf(b):
                return math.inf
            d = max(abs(a), abs(b))
            return float(abs(a - b) / d) if d > 0 else 0.0

        improved = obj < opt_obj
        conv = (res_prim < t_prim and res_dual < t_dual) or (res_comb < t_comb)
        done = bool(conv and not fixed_iters)
        grow = res_comb > last_res * mp.mpf(0.9)
        margin = min(dist(obj, opt_obj), dist(res_prim, t_prim), dist(res_dual, t_dual), dist(res_comb, t_comb))
        if not done:
            margin = min(margin, dist(res_comb, last_res * mp.mpf(0.9)))
        return dict(improved=bool(improved), opt_obj=float(obj if improved else opt_obj), conv=bool(conv), done=done,
                    mu=float(mu) if done or not grow else float(mu) * float(rho), grow=bool(grow),
                    last_res=float(last_res) if done else float(res_comb), res_comb=float(res_comb),
                    res_prim=float(res_prim), res_dual=float(res_dual), t_prim=float(t_prim), t_dual=float(t_dual),
                    t_comb=float(t_comb), margin=margin)


# ---------------------------------------------------------------- (b) known-answer inputs
def hadamard(k):
    """Sylvester-Hadamard matrix of order k (a power of two), integer entries."""
    H = np.array([[1]], dtype=np.int64)
    while H.shape[0] < k:
        H = np.block([[H, H], [H, -H]])
    if H.shape[0] != k:
        raise ValueError("the order must be a power of two")
    return H


@dataclass
class KnownAnswer:
    E: np.ndarray          # tx x rx complex f64, exact
    lam: list              # eigenvalues of E E^H (Fractions), in the order of s (zero-padded to tx)
    Q: np.ndarray          # tx x tx: column i the eigenvector of lam[i] (exact in f64 when tx is a power of 4)
    left: object           # D1 P1 Hd as complex integer matrix (numpy object arrays are avoided: int64)
    right: object          # Hd'^T P2 D2
    s: list
    k: int


def known_answer(tx, rx, s, seed=0, k=None):
    """E = D1 P1 Hd diag(s) Hd'^T P2 D2 / 2^k with integer s (len <= min(tx, rx)); the permutations and the
    {+-1, +-j} diagonals are drawn from ``seed``.  k defaults to floor(log2(tx rx) / 2)."""
    rng = np.random.default_rng(seed)
    s = [int(v) for v in s] + [0] * (min(tx, rx) - len(s))
    if k is None:
        k = int(math.log2(tx * rx)) // 2
    units = np.array([1, 1j, -1, -1j])
    d1, d2 = units[rng.integers(0, 4, tx)], units[rng.integers(0, 4, rx)]
    p1, p2 = rng.permutation(tx), rng.permutation(rx)
    left = d1[:, None] * hadamard(tx)[p1, :]                       # D1 P1 Hd
    right = (hadamard(rx).T[:, p2]) * d2[None, :]                  # Hd'^T P2 D2
    S = np.zeros((tx, rx))
    for i, v in enumerate(s):
        S[i, i] = v
    E = (left @ S @ right) / 2.0 ** k                              # integer sums below 2^53: exact
    assert np.abs(left @ np.abs(S) @ np.abs(right)).max() < 2.0 ** 52
    lam = [Fraction(v * v * tx * rx, 4 ** k) for v in s] + [Fraction(0)] * (tx - len(s))
    Q = left / math.sqrt(tx)
    return KnownAnswer(E=np.ascontiguousarray(E.astype(np.complex128)), lam=lam, Q=np.ascontiguousarray(Q), left=left,
                       right=right, s=s, k=k)


def known_answer_z(ka, rl, fl):
    """Z of a known-answer input without an eigensolver: the profile loop in Fractions on the exact eigenvalues,
    one square root per group at DPS digits.  Returns (Z as an mp matrix, scale per eigenvalue in the order of
    ka.lam (Fractions), fired flags, margin)."""
    tx, rx = ka.E.shape
    order = sorted(range(tx), key=lambda i: -ka.lam[i])            # stable descending
    lam = [ka.lam[i] for i in order]
    sc, fired, _, margin = profile_loop(lam, rl, fl, num=Fraction)
    scale = [Fraction(1)] * tx
    for kpos, i in enumerate(order):
        scale[i] = sc[kpos]
    with mp.workdps(DPS):
        roots = {}
        Z = mp.matrix(tx, rx)
        L = ka.left
        R = ka.right
        for i, sv in enumerate(ka.s):
            if sv == 0:
                continue
            c = scale[i]
            if c not in roots:
                roots[c] = mp.sqrt(mp.mpf(c.numerator) / mp.mpf(c.denominator))
            wgt = roots[c] * sv / mp.mpf(2) ** ka.k
            for a in range(tx):
                la = L[a, i]
                la = mp.mpc(int(la.real), int(la.imag))
                for b in range(rx):
                    rb = R[i, b]
                    Z[a, b] += wgt * la * mp.mpc(int(rb.real), int(rb.imag))
        return Z, scale, fired, margin


def ref_z_mp(ref):
    """The general reference's Z as an mp matrix (for the 1e-30 comparison with a known answer)."""
    with mp.workdps(DPS):
        tx, cols = ref.E.shape
        Z = mp.matrix(tx, cols)
        for i in range(tx):
            for j in range(cols):
                Z[i, j] = mp.mpc(mp.mpf(float(ref.Z_hi[i, j].real)) + mp.mpf(float(ref.Z_lo[i, j].real)),
                                 mp.mpf(float(ref.Z_hi[i, j].imag)) + mp.mpf(float(ref.Z_lo[i, j].imag)))
        return Z


def share_spectrum(tx, r, f, delta, tail_seed=0, bits=34):
    """Integer s (length tx) whose top-r share of sum s^2 is f (1 + delta) as closely as integers of `bits` bits
    allow: the tail is drawn at random, the r top values are equal up to the last one, which is tuned."""
    rng = np.random.default_rng(tail_seed)
    tail = [int(v) for v in rng.integers(1 << (bits - 6), 1 << (bits - 4), tx - r)]
    T = sum(v * v for v in tail)
    share = Fraction(f) * (1 + Fraction(delta))
    top2 = share * T / (1 - share)                   # required sum of the top r squares
    each = math.isqrt(int(top2 / r))
    top = [each + 7 * (r - 1 - i) for i in range(r - 1)]   # distinct, descending
    rest = top2 - sum(v * v for v in top)
    last = math.isqrt(int(rest))
    top.append(last)
    top.sort(reverse=True)
    assert top[-1] > max(tail)
    return top + sorted(tail, reverse=True)


# ---------------------------------------------------------------- numpy models of a wrong Z-step
MUTANTS = ("off1", "nosqrt", "ties", "unscaled", "f32scale")


def z_model(E, rl, fl, kind=None):
    """ArgMinZ in f64 numpy, right (kind None) or wrong in one way: 'off1' the group boundary one too far,
    'nosqrt' scale instead of sqrt(scale), 'ties' a descending rank without the tie-break (equal clamped
    eigenvalues get the same position, so the order is no permutation; the positions left over hold a stale
    index, here the top eigenvalue's: with a valid permutation the order inside a tie cannot change a
    well-posed Z, so this is the form in which such a fault shows), 'unscaled' a later profile entry
    reads the unscaled spectrum, 'f32scale' sqrt(scale) rounded to f32.  Returns (Z, scale per eigen index)."""
    tx = E.shape[0]
    H = E @ E.conj().T
    H = 0.5 * (H + H.conj().T)
    w, Uv = np.linalg.eigh(H)
    s2 = np.maximum(0.0, w)
    idx = np.argsort(-s2, kind="stable")
    if kind == "ties":
        idx = np.full(tx, int(np.argmax(s2)), dtype=np.int64)
        for i in range(tx):
            idx[int(np.sum(s2 > s2[i]))] = i
    s2s = s2[idx].copy()
    s2o = s2s.copy()
    sc = np.ones(tx)
    for rr, f in zip(rl, fl):
        src = s2o if kind == "unscaled" else s2s
        vr, v = float(np.cumsum(src[:rr])[-1]), float(np.cumsum(src)[-1])
        if vr < v * f:
            c = min(1.0, vr / (v - vr) * (1.0 / f - 1.0))
            k0 = rr + 1 if kind == "off1" else rr
            s2s[k0:] *= c
            np.multiply.at(sc, idx[k0:], c)
    if not np.any(sc < 1):
        return E.copy(), sc
    d = sc if kind == "nosqrt" else np.sqrt(sc)
    if kind == "f32scale":
        d = np.sqrt(sc).astype(np.float32).astype(np.float64)
    return (Uv * d[None, :]) @ Uv.conj().T @ E, sc


def model_applies(kind, sc_right, sc_wrong):
    """Whether an input exercises a fault of ``z_model``: a rescaling fires in the right model and the wrong
    one applies other factors ('nosqrt', 'f32scale': other functions of the same factors)."""
    if not np.any(sc_right < 1):
        return False
    return kind in ("nosqrt", "f32scale") or not np.allclose(sc_right, sc_wrong, rtol=1e-9, atol=0.0)


# ---------------------------------------------------------------- the suite's inputs
def profile_of(tx, rx, kind):
    """kind: 'full' (m < 3n: rank_profile's [3,4,6,12] / [3,4,6] / [3,4,8] / [2] / ...), 'm3n' ([r3] / [0.995]),
    'r1' (rank one)."""
    n = tx * rx
    if kind == "r1":
        return O.rank_profile(tx, rx, n, n, 1)
    return O.rank_profile(tx, rx, 3 * n if kind == "m3n" else n, n, 0)


def m_of(tx, rx, kind):
    return 3 * tx * rx if kind == "m3n" else tx * rx


def lowrank_noise(tx, cols, L, noise, seed):
    """Rank-|L| signal plus Gaussian noise of relative level `noise` (full mantissas); path gains 1 / (1 + i), or
    equal gains for L < 0 (a flat top group: the first profile entry fires before the later ones)."""
    rng = np.random.default_rng(seed)
    g = 1.0 / (1.0 + np.arange(abs(L))) if L > 0 else np.ones(abs(L))
    L = abs(L)
    a = np.linalg.qr(rng.standard_normal((tx, L)) + 1j * rng.standard_normal((tx, L)))[0]
    b = np.linalg.qr(rng.standard_normal((cols, L)) + 1j * rng.standard_normal((cols, L)))[0]
    S = (a * g[None, :]) @ b.conj().T               # singular values g
    Nz = rng.standard_normal((tx, cols)) + 1j * rng.standard_normal((tx, cols))
    return S / np.linalg.norm(S) * math.sqrt(tx * cols) + noise * Nz


@dataclass(frozen=True)
class Case:
    """One batch of the suite: realisation b is lowrank_noise(tx, r rx, L[b], noise[b], seed + b)."""
    name: str
    tx: int
    rx: int
    r: int
    kind: str          # profile kind
    L: tuple           # per realisation (negative: equal path gains)
    noise: tuple       # per realisation
    seed: int
    want: tuple = ()   # intended firing pattern per realisation: 'none' | 'first' | 'all' | 'some'

    @property
    def batch(self):
        return len(self.noise)

    @property
    def n(self):
        return self.tx * self.rx

    def profile(self):
        return profile_of(self.tx, self.rx, self.kind)

    def m(self):
        return m_of(self.tx, self.rx, self.kind)

    def X(self):
        """[batch][r][n] complex f64."""
        return np.stack([from_E(lowrank_noise(self.tx, self.r * self.rx, L, nz, self.seed + b), self.r)
                         for b, (L, nz) in enumerate(zip(self.L, self.noise))])


def pattern(ref):
    """'none' | 'first' | 'all' | 'some' from a reference's fired flags (clamped entries count as not fired)."""
    if not ref.any_fired:
        return "none"
    if all(ref.fired):
        return "all"
    if ref.fired[0] and not any(ref.fired[1:]):
        return "first"
    return "some"


@functools.lru_cache(maxsize=None)
def case_refs(case):
    """The references of a case's realisations with N = 0 (E = X), computed once per process."""
    rl, fl = case.profile()
    X = case.X()
    return tuple(argmin_z_ref(to_E(X[b], case.tx), rl, fl) for b in range(case.batch))


def _c(name, tx, rx, r, kind, L, noise, seed, want):
    return Case(name, tx, rx, r, kind, tuple(L), tuple(noise), seed, tuple(want))


# one-wave kernel (r = 1): every shape of the issue with its rank_profile, the m >= 3n and rank-one profiles;
# each batch mixes the firing patterns, every realisation has its own spectrum
CASES_1W = (
    _c("2x2", 2, 2, 1, "full", (1, 1, 2), (0.1, 0.5, 1.0), 100, ("none", "none", "none")),
    _c("4x4", 4, 4, 1, "full", (1, 1, 1), (0.2, 1.0, 1.6), 110, ("none", "all", "all")),
    _c("8x8", 8, 8, 1, "full", (2, 2, 3), (0.1, 0.5, 1.5), 120, ("none", "all", "all")),
    _c("16x16", 16, 16, 1, "full", (3, -4, 3), (0.05, 0.01, 0.5), 130, ("none", "first", "all")),
    _c("16x8", 16, 8, 1, "full", (2, 2, 3), (0.1, 0.4, 1.0), 140, ("none", "all", "all")),
    _c("8x32", 8, 32, 1, "full", (2, 2, 3), (0.1, 0.4, 1.0), 150, ("none", "all", "all")),
    _c("32x32", 32, 32, 1, "full", (3, -4, 3), (0.05, 0.01, 0.6), 160, ("none", "first", "all")),
    _c("16x16-m3n", 16, 16, 1, "m3n", (3, 3, 3), (0.05, 0.3, 1.0), 170, ("none", "all", "all")),
    _c("8x32-m3n", 8, 32, 1, "m3n", (2, 2, 3), (0.05, 0.5, 1.5), 180, ("none", "all", "all")),
    _c("16x16-some", 16, 16, 1, "full", (3, 3, 3), (0.2, 0.3, 0.17), 190, ("some", "some", "some")),
)
CASES_R1 = (
    _c("16x16-r1", 16, 16, 1, "r1", (1, 1, 2), (0.05, 0.3, 1.0), 200, ("none", "all", "all")),
    _c("32x32-r1", 32, 32, 1, "r1", (1,), (0.3,), 211, ("all",)),
    _c("2x2-r1", 2, 2, 1, "r1", (1, 1, 2), (0.05, 0.5, 1.0), 230, ("none", "all", "all")),
    _c("8x8-r1", 8, 8, 1, "r1", (1, 1, 2), (0.05, 0.4, 1.0), 220, ("none", "all", "all")),
)
# 65 realisations (ragged groups of 4 and 8), noise from certifiable to fully rescaled
CASE_B65 = _c("8x8-b65", 8, 8, 1, "full", [1 + b % 3 for b in range(65)], [0.03 + 0.025 * b for b in range(65)], 300,
              ())
# four-wave kernel (r > 1): the tx, rx <= 16 per-wave form and the 32 x 32 form
CASES_4W = (
    _c("16x16-r2", 16, 16, 2, "full", (3, -4, 3), (0.05, 0.01, 0.5), 400, ("none", "first", "all")),
    _c("8x8-r5", 8, 8, 5, "full", (2, 2, 3), (0.1, 0.5, 1.5), 410, ("none", "all", "all")),
    _c("16x8-r20", 16, 8, 20, "full", (2, 2, 3), (0.1, 0.4, 1.0), 420, ("none", "all", "all")),
    _c("4x4-r32", 4, 4, 32, "full", (1, 1, 2), (0.2, 1.0, 2.5), 430, ("none", "all", "all")),
    _c("32x32-r2", 32, 32, 2, "full", (3, -4, 3), (0.05, 0.01, 0.6), 440, ("none", "first", "all")),
    _c("8x32-r5", 8, 32, 5, "full", (2, 2, 3), (0.1, 0.4, 1.0), 450, ("none", "all", "all")),
    _c("32x32-r20", 32, 32, 20, "full", (3,), (0.6,), 469, ("all",)),
    _c("8x32-r32", 8, 32, 32, "m3n", (2,), (0.6,), 470, ("all",)),
)
ALL_CASES = CASES_1W + CASES_R1 + (CASE_B65,) + CASES_4W


# ---------------------------------------------------------------- known-answer inputs of the suite
CERT_DELTAS = (1e-3, 1e-6, 1e-8)
CERT_KINDS = ("m3n", "r1")      # single-entry profiles: [8] / [0.995] and [1] / [0.95] at 16 x 16
CERT_T = 16


@functools.lru_cache(maxsize=None)
def cert_input(kind, delta):
    """16 x 16 known-answer input whose top-group share vr / v is f (1 + delta) (delta of either sign); the pair
    (+delta, -delta) shares its tail, permutations and diagonals, so the two differ by a perturbation of relative
    size ~|delta|.  Q (exact in f64: tx is a power of 4) holds the eigenvectors in descending eigenvalue order."""
    rl, fl = profile_of(CERT_T, CERT_T, kind)
    s = share_spectrum(CERT_T, rl[0], fl[0], delta, tail_seed=5)
    return known_answer(CERT_T, CERT_T, s, seed=17)


def top_share(ka, r):
    """Exact top-r share of the eigenvalue sum (a Fraction)."""
    lam = sorted(ka.lam, reverse=True)
    return sum(lam[:r]) / sum(lam)


@functools.lru_cache(maxsize=None)
def degenerate_inputs():
    """name -> (KnownAnswer, profile kind): a triple top eigenvalue inside group 1-3 (well-posed), a tie across the
    first boundary (lambda_3 = lambda_4 with r_0 = 3: Z itself is ill-posed), rank one, and the first input scaled
    by 2^+-332 (about 1e+-100)."""
    out = {}
    out["triple"] = (known_answer(16, 16, [900, 900, 900, 500, 410, 330, 250, 200, 150, 120, 90, 70, 50, 30, 20, 10],
                                  seed=21), "full")
    out["straddle"] = (known_answer(16, 16, [900, 800, 600, 600, 410, 330, 250, 200, 150, 120, 90, 70, 50, 30, 20, 10],
                                    seed=22), "full")
    out["rank1"] = (known_answer(16, 16, [1000], seed=23), "full")
    for name, e in (("huge", 332), ("tiny", -332)):
        ka = known_answer(16, 16, [900, 700, 650, 500, 410, 330, 250, 200, 150, 120, 90, 70, 50, 30, 20, 10], seed=24)
        ka.E = np.ldexp(ka.E.real, e) + 1j * np.ldexp(ka.E.imag, e)
        ka.lam = [v * Fraction(4) ** e for v in ka.lam]
        ka.k -= e
        out[name] = (ka, "full")
    return out


OUT_OF_BAND = {"huge": 332, "tiny": -332}     # |E| about 1e+-100: tr(E E^H) far outside [2^-400, 2^400]


@functools.lru_cache(maxsize=None)
def out_of_band_pair(name):
    """Two 16 x 16 known-answer inputs with different spectra, permutations and diagonals, scaled by 2^+-332:
    E = [E0 | E0'] is a two-column iterate (r = 2) for the four-wave kernel, E0 alone one for the one-wave kernel."""
    e = OUT_OF_BAND[name]
    k0 = known_answer(16, 16, [900, 700, 650, 500, 410, 330, 250, 200, 150, 120, 90, 70, 50, 30, 20, 10], seed=24)
    k1 = known_answer(16, 16, [800, 760, 300, 280, 260, 240, 220, 200, 180, 160, 140, 120, 100, 80, 60, 40], seed=25)
    sc = lambda E: np.ldexp(E.real, e) + 1j * np.ldexp(E.imag, e)   # noqa: E731
    return sc(k0.E), sc(k1.E)
