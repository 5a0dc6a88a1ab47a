"""Exact references and derived tolerances for the four linear operators of the ADMM iteration
(tests/test_gpu_linops.py; self-tested on the CPU by tests/test_linop_ref.py).

    T  = (Y - M/mu) - A (Z - N/mu)        X = (Z - N/mu) + A^H g        KY = K Y        g = G T

Exact products
--------------
All operands are f64, so every product is an exact rational.  ``exact_matvec`` evaluates it without
rounding: each row of the (real-expanded) matrix and each vector is scaled by a power of two below 1 and
cut into 20-bit integer slices (six per vector, as many as a row's entries need); a product of two slices
summed over at most 2^11 terms stays below 2^51, so the f64 matmul of two slice planes is exact.  The
planes are recombined in Python integers, multiplied by the integer mantissa of an optional f64 scale (the
phase-code factor c), and returned as an unevaluated sum hi + lo of two f64.  What the six vector slices
cut off lies below 2^-120 of the vector's largest component, i.e. more than 2^60 below every tolerance
here.  Errors against the reference are formed with ``math.fsum`` (exact summation, one final rounding).

V = fma(-N, 1/mu, Z) and S = fma(-M, 1/mu, Y) are reproduced as the int8 kernels define them: the correctly
rounded value of the exact Z - N fl(1/mu) (``fma_ref``, through ``fractions.Fraction``).  The tolerances
below then cover the product and the final additions only; the f64 kernels, which may round N/mu before
the subtraction, get that second rounding as an explicit term.

int8 digit planes (csrc/ace_i8.hpp, ace_i8gemm.hip), per real output of vector j
---------------------------------------------------------------------------------
    tol = c N_nz 2^(e_j - 55) (1 + 2^-9) + gamma_8 |exact| + u (|S| + |T|)
e_j = ilogb(bound_j) + 1 (``exp_of``), clamped to [-960, 1000], is the kernel's exponent: each component is
rounded to a multiple of 2^(e - 54), an error of at most 2^(e - 55) per component, and N_nz of them enter
the output with weight c (N_nz: the nonzero entries of that row of the real expansion of P + jQ: n for a
phase code, 2n for c(+-1 +-j); for K Y the absolute row sum of K_int and c^2).  The integer plane sums are
exact; the Horner recombination is 7 fmas and the scale one multiply: gamma_8 = 8u / (1 - 8u) on the result,
plus u times the excess of the Horner partial sums over the result, at most N_nz 128^6 (1 + 1/127) units
of c 2^(e - 54), which is the 2^-9 above.  S - (A V) (or V + W) is one more rounding: u |T|; u |S| is the
issue's allowance for the epilogue operand.  u = 2^-53.

f64 3M matrix-core GEMM / GEMV (ace_gemm.hip, ace_gemv.hip), per real output
-----------------------------------------------------------------------------
    tol = 2 (K + 4) u sum_k (|a_r| + |a_i|)(|v_r| + |v_i|) + u (|E| + |C|)  [+ operand roundings]
Three dot products of length K (P1 = v_r a_r, P2 = v_i a_i, P3 = (v_r + v_i)(a_r + a_i)), each within
gamma_K of its absolute sum (Higham, Accuracy and Stability, (3.5)), the two pre-additions (one rounding on
each factor of P3) and the two subtractions of the recombination: every absolute sum is at most
sum (|a_r| + |a_i|)(|v_r| + |v_i|), and Im = P3 - P1 - P2 carries all three, hence 2 (K + 4) u to first order.
Where a kernel forms V = Z - N/mu or S = Y - M/mu with a rounded quotient, ``pre_rounding`` adds
2u |N/mu| (propagated through sum |a|) and 2u |M/mu|.

G = (I + K)^-1 by Newton-Schulz (ace_admm.cpp: ns_inverse)
----------------------------------------------------------
    || g - g* ||_inf <= gamma_m kappa_inf(I + K) || g* ||_inf,      g* the longdouble solution of (I + K) g = T
With B = I + K, the last step forms S = I - X B (computed: S + d1) and G = X + X (S + d1)^H + d2, so
    G - B^-1 = -S^2 B^-1 + X d1^H + d2,          g - g* = (G - B^-1) T.
The stopping rule runs one step after max|S_ij| < 1e-10, so ||S^2||_inf <= (m 1e-10)^2.  d1 is the GEMM
rounding of X B: |d1| <= gamma_g |X||B| + u with gamma_g = 2 (m + 4) u, so ||d1||_inf <= gamma_g kappa_inf + u
(X = B^-1 to first order); d2 is the rounding of the second GEMM and of the Hermitian average,
||d2||_inf <= (gamma_g 1e-10 m + 3u) ||X||_inf.  Hence
    || g - g* ||_inf <= [ (m 1e-10)^2 + gamma_g kappa_inf + 4u ] ||B^-1||_inf ||T||_inf.
This is the statement the tests assert on vectors T that attain ||B^-1 T||_inf = ||B^-1||_inf ||T||_inf (the
sign vector of a row of B^-1), where it reads as the issue's form with
    gamma_m = gamma_g + ((m 1e-10)^2 + 4u) / kappa_inf  <=  gamma_g + (m 1e-10)^2 + 4u   (kappa >= 1),
and, with the same gamma_m, on random T (for which ||g*|| may be smaller than ||B^-1|| ||T||: the bound is
then tighter than what the argument above proves, and is asserted as the issue states it).  The apply
g = G T itself adds the GEMM tolerance against the exact product of the G read back from the setup.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
SLICE = 20
NSL_V = 6


# ---------------------------------------------------------------- exact arithmetic helpers
def real_expand(A):
    """Real expansion E of a complex matrix: (E x)(interleaved re, im) = A x."""
    A = np.asarray(A)
    R, C = A.shape
    E = np.zeros((2 * R, 2 * C))
    E[0::2, 0::2] = A.real
    E[0::2, 1::2] = -A.imag
    E[1::2, 0::2] = A.imag
    E[1::2, 1::2] = A.real
    return E


def _slices(X, nsl):
    """Rows of X scaled by 2^-e_row (|x| < 1) and cut into nsl SLICE-bit integer planes (f64 integers);
    returns (planes, e_row).  Exact when the row's entries span at most nsl * SLICE bits below its maximum."""
    X = np.asarray(X, dtype=np.float64)
    mx = np.max(np.abs(X), axis=1)
    e = np.where(mx > 0, np.frexp(mx)[1], 0).astype(np.int64)
    x = np.ldexp(X, (-e)[:, None])
    planes = []
    for _ in range(nsl):
        x = x * float(1 << SLICE)
        t = np.trunc(x)   # (towards zero: x - t keeps x's sign and needs no new bits, so it is exact)
        planes.append(t)
        x = x - t
        if not x.any():
            break
    return planes, e


def _split_int(t):
    """(hi, lo) f64 with hi + lo = the Python integer t to 2^-106 relative (hi correctly rounded)."""
    hi = float(t)
    return hi, float(t - int(hi))


def exact_matvec(E, V, scale=1.0):
    """scale * E V^T for a real matrix E [R][C] and real vectors V [nv][C], as (hi, lo) f64 arrays
    [nv][R] with hi + lo equal to the exact value (see the module docstring)."""
    E = np.asarray(E, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    assert E.shape[1] == V.shape[1] and E.shape[1] <= 2048 + 2048
    assert np.isfinite(E).all() and np.isfinite(V).all()
    ep, ee = _slices(E, 6)
    vp, ve = _slices(V, NSL_V)
    nv, R = V.shape[0], E.shape[0]
    # sum over slice pairs of (E_a V_b^T) 2^(-SLICE (a + b + 2)); everything in units of 2^(-SLICE (na + nb))
    na, nb = len(ep), len(vp)
    tot = np.zeros((nv, R), dtype=object)
    for a in range(na):
        for b in range(nb):
            P = vp[b] @ ep[a].T   # exact: |sum| < 2^(2 SLICE + 12) <= 2^52
            sh = SLICE * ((na - 1 - a) + (nb - 1 - b))
            tot = tot + (P.astype(np.int64).astype(object) << sh if sh else P.astype(np.int64).astype(object))
    sm, sx = math.frexp(float(scale))
    smi = int(math.ldexp(sm, 53))   # scale = smi 2^(sx - 53)
    tot = tot * smi
    sp = np.frompyfunc(_split_int, 1, 2)
    hi, lo = sp(tot)
    ex = (ve[:, None] + ee[None, :]) - SLICE * (na + nb) + (sx - 53)
    return np.ldexp(hi.astype(np.float64), ex), np.ldexp(lo.astype(np.float64), ex)


def exact_cmatvec(A, V, scale=1.0, herm=False):
    """scale * A V (or A^H V) for a complex matrix and complex vectors V [nv][cols]: (hi, lo) as complex-
    interleaved f64 arrays [nv][2 rows]."""
    A = np.asarray(A, dtype=np.complex128)
    if herm:
        A = A.conj().T
    V = np.ascontiguousarray(np.asarray(V, dtype=np.complex128))
    return exact_matvec(real_expand(A), V.view(np.float64), scale)


_fsum_abs = np.frompyfunc(lambda *a: abs(math.fsum(a)), 4, 1)


def _reals(X):
    return np.ascontiguousarray(np.asarray(X, np.complex128)).view(np.float64)


def err_against(out, hi, lo, add=None, sign=1):
    """|out - (add + sign (hi + lo))| per real component, formed exactly (one rounding); out complex [nv][k],
    hi / lo interleaved reals [nv][2k], add (complex or None) an exactly known f64 addend."""
    o = _reals(out)
    a = np.zeros_like(o) if add is None else _reals(add)
    return _fsum_abs(o, -a, -sign * hi, -sign * lo).astype(np.float64)


def fma_ref(Nv, imu_v, Z):
    """fma(-N, imu, Z) per real component: the correctly rounded exact Z - N imu (complex [nv][k] in / out,
    imu_v [nv] the f64 reciprocals 1/mu as the kernels form them)."""
    Nr, Zr = _reals(Nv), _reals(Z)
    out = Zr.copy()
    for j, k in zip(*np.nonzero(Nr)):
        n, z, i = float(Nr[j, k]), float(Zr[j, k]), float(imu_v[j])
        if math.isfinite(n) and math.isfinite(z) and math.isfinite(i):
            out[j, k] = float(Fraction(z) - Fraction(n) * Fraction(i))
        else:
            out[j, k] = z - n * i
    return out.view(np.complex128)


def per_vector(x, nv, rcols=1):
    """A per-realisation array broadcast to the nv = batch * rcols vectors."""
    return np.repeat(np.broadcast_to(np.asarray(x, np.float64), (nv // rcols,)), rcols)


# ---------------------------------------------------------------- phase codes
def phase_parts(A):
    """(c, P, Q) of a phase-code matrix A = c (P + jQ), P, Q in {-1, 0, 1} (integer arrays)."""
    A = np.asarray(A, np.complex128)
    c = float(np.max(np.abs(A.view(np.float64))))
    P, Q = A.real / c, A.imag / c
    assert np.isin(P, (-1.0, 0.0, 1.0)).all() and np.isin(Q, (-1.0, 0.0, 1.0)).all()
    return c, P.astype(np.int64), Q.astype(np.int64)


def kint(A):
    """The Gaussian-integer matrix K_int = (P + jQ)(P + jQ)^H as (real, imag) int64 arrays."""
    _, P, Q = phase_parts(A)
    return P @ P.T + Q @ Q.T, Q @ P.T - P @ Q.T


def kernel_exp(bound):
    """exp_of (csrc/ace_i8.hpp): the digit exponent of a finite bound."""
    bound = np.asarray(bound, np.float64)
    e = np.where(bound > 0, np.frexp(np.where(bound > 0, bound, 1.0))[1], 0)   # ilogb + 1 = frexp exponent
    return np.clip(e, -960, 1000).astype(np.int64)


def maxabs_rows(X):
    return np.max(np.abs(np.ascontiguousarray(np.asarray(X, np.complex128)).view(np.float64)), axis=1)


GAMMA8 = 8 * U / (1 - 8 * U)


def i8_tol(Eint, scale, e, exact_hi, S=None, T=None):
    """The int8 tolerance per real output [nv][R]: Eint the integer real expansion [R][C] (its absolute row
    sums are N_nz), scale = c (or c^2), e [nv] the kernel's exponents, exact_hi the exact product, S / T the
    epilogue operand and the result (complex or None)."""
    nnz = np.abs(np.asarray(Eint)).sum(axis=1).astype(np.float64)
    base = scale * nnz[None, :] * np.ldexp(1.0, np.asarray(e) - 55)[:, None] * (1 + 2.0 ** -9)
    tol = base + GAMMA8 * np.abs(exact_hi)
    for X in (S, T):
        if X is not None:
            tol = tol + U * np.abs(np.ascontiguousarray(np.asarray(X, np.complex128)).view(np.float64))
    return tol


def uniform_rms(Eint, scale, e):
    """RMS of the product's error under uniform rounding of each component to 2^(e - 54):
    c sqrt(N_nz / 12) 2^(e - 54), per real output [nv][R]."""
    nnz = np.abs(np.asarray(Eint)).sum(axis=1).astype(np.float64)
    return scale * np.sqrt(nnz / 12.0)[None, :] * np.ldexp(1.0, np.asarray(e) - 54)[:, None]


def digit_model(Eint, scale, V, e, drop_low=False, cut_shift=0, scale_shift=0):
    """Integer numpy model of the digit scheme for real vectors V [nv][C]: round to 2^(e - 54), exact integer
    product, one rounding to f64, scale.  Faults: drop_low loses the lowest digit plane (7 bits); cut_shift
    moves the exponent of both the cut and the scale (the 56-bit two's-complement digit image wraps);
    scale_shift moves the exponent of the scale alone."""
    V = np.asarray(V, np.float64)
    Ei = np.asarray(Eint).astype(np.int64).astype(object)
    out = np.empty((V.shape[0], Ei.shape[0]))
    for j in range(V.shape[0]):
        ej = int(e[j]) + cut_shift
        wi = [int(x) for x in np.rint(np.ldexp(V[j], 54 - ej))]
        wi = [((x + (1 << 55)) % (1 << 56)) - (1 << 55) for x in wi]
        if drop_low:
            wi = [x - (x % 128) for x in wi]
        s = Ei @ np.array(wi, dtype=object)
        out[j] = [math.ldexp(float(x), ej + scale_shift - 54) * scale for x in s]
    return out


# ---------------------------------------------------------------- f64 3M GEMM
def gemm_tol(A, V, E=None, C=None, herm=False):
    """2 (K + 4) u sum_k (|a_r| + |a_i|)(|v_r| + |v_i|) per complex output, repeated for its two real
    components [nv][2 rows], plus u (|E| + |C|)."""
    A = np.asarray(A, np.complex128)
    if herm:
        A = A.conj().T
    V = np.asarray(V, np.complex128)
    K = A.shape[1]
    a1 = np.abs(A.real) + np.abs(A.imag)
    v1 = np.abs(V.real) + np.abs(V.imag)
    tol = np.repeat(2 * (K + 4) * U * (v1 @ a1.T), 2, axis=1)
    for X in (E, C):
        if X is not None:
            tol = tol + U * np.abs(np.ascontiguousarray(np.asarray(X, np.complex128)).view(np.float64))
    return tol


def pre_rounding(A, Nv, imu_v, herm=False):
    """Allowance for a V = Z - N/mu formed with a rounded quotient (two roundings instead of the fma's one):
    2u |N/mu| carried through sum_k |a| per real output [nv][2 rows]."""
    A = np.asarray(A, np.complex128)
    if herm:
        A = A.conj().T
    Nv = np.asarray(Nv, np.complex128)
    q = (np.abs(Nv.real) + np.abs(Nv.imag)) * np.asarray(imu_v)[:, None]
    a1 = np.abs(A.real) + np.abs(A.imag)
    return np.repeat(2 * U * (q @ a1.T), 2, axis=1)


def own_rounding(Nv, imu_v):
    """2u |N/mu| per real component: the same allowance for an epilogue operand S = Y - M/mu or V."""
    return 2 * U * np.abs(_reals(Nv)) * np.asarray(imu_v)[:, None]


def gemm3m_model(A, V, herm=False):
    """numpy emulation of the 3M product in f64 (sequential accumulation over k): A V per vector."""
    A = np.asarray(A, np.complex128)
    if herm:
        A = A.conj().T
    V = np.asarray(V, np.complex128)
    ar, ai, vr, vi = A.real, A.imag, V.real, V.imag
    as_, vs = ar + ai, vr + vi
    p1 = np.zeros((V.shape[0], A.shape[0]))
    p2 = np.zeros_like(p1)
    p3 = np.zeros_like(p1)
    for k in range(A.shape[1]):
        p1 += vr[:, k:k + 1] * ar[None, :, k]
        p2 += vi[:, k:k + 1] * ai[None, :, k]
        p3 += vs[:, k:k + 1] * as_[None, :, k]
    return (p1 - p2) + 1j * (p3 - p1 - p2)


# ---------------------------------------------------------------- G
def ninf(Mx):
    """Infinity norm of a complex matrix (vector: of its moduli)."""
    Mx = np.abs(np.asarray(Mx))
    return float(np.max(np.sum(Mx, axis=-1))) if Mx.ndim == 2 else float(np.max(Mx))


def g_reference(K, T):
    """(g*, kappa_inf(I + K), B^-1 in f64) for B = I + K (Hermitian, eigenvalues >= 1): g* [nv][m] solves
    B g = T to longdouble accuracy (f64 inverse, then iterative refinement with longdouble residuals: each
    step multiplies the error by about kappa u, three steps reach the longdouble rounding level)."""
    K = np.asarray(K, np.complex128)
    m = K.shape[0]
    B = np.eye(m) + K
    Binv = np.linalg.inv(B)
    Bl = B.astype(np.clongdouble)
    Tl = np.asarray(T, np.clongdouble)
    g = (Binv @ np.asarray(T, np.complex128).T).T.astype(np.clongdouble)
    for _ in range(3):
        r = Tl - (Bl @ g.T).T
        g = g + (Binv @ r.astype(np.complex128).T).T.astype(np.clongdouble)
    r = Tl - (Bl @ g.T).T
    lim = 4 * m * float(np.finfo(np.longdouble).eps)   # (the longdouble residual's own rounding level)
    assert ninf(r.astype(np.complex128)) <= lim * ninf(B) * max(ninf(g.astype(np.complex128)), 1e-300), "refinement"
    return g, ninf(B) * ninf(Binv), Binv


def norm_attaining(Binv, rows):
    """Unit-modulus vectors T_i with (B^-1 T_i)_i = sum_k |B^-1_ik|, for the rows i whose absolute sum is
    largest: ||B^-1 T||_inf = ||B^-1||_inf ||T||_inf on the first of them."""
    order = np.argsort(-np.sum(np.abs(Binv), axis=1))[:rows]
    ph = np.angle(Binv[order])
    return np.exp(-1j * ph)


def gamma_m(m):
    """gamma_m of the module docstring (the kappa >= 1 form)."""
    return 2 * (m + 4) * U + (m * 1e-10) ** 2 + 4 * U


def gamma_gj(m):
    """Private codebooks: Gauss-Jordan without pivoting on the Hermitian positive definite B (no growth).  Each
    of the m elimination steps updates an entry with one multiply-add (2 roundings) and the pivot row with one
    division; the computed inverse is that of a matrix within 2 m u |L||U|-type perturbations on either side
    of the elimination (forward and backward sweeps run together), i.e. 8 m u in the kappa form, first order."""
    return 8 * m * U


# ---------------------------------------------------------------- codebooks and data recipes of the tests
def codebook(kind, m, n, seed=0):
    """Phase-code test codebooks A = c (P + jQ) [m][n]:
    "synth"  the package's synthetic code j^k / sqrt(n);   "off"  the same with a third of the antennas off;
    "pmj1"   (+-1 +-j), c = 1;   "pmj"  (+-1 +-j), c = 1 / sqrt(2n);
    "twin"   (+-1 +-j) / 32 with rows 0 and 1 all (1 + j): K_int[0][1] = 2n."""
    rng = np.random.default_rng([seed, m, n, len(kind)])
    if kind in ("synth", "off"):
        from ace_amd import synth
        k = synth.codebook_codes(1234 + seed, m, n).astype(np.int64)
        P = np.array([1, 0, -1, 0])[k % 4]
        Q = np.array([0, 1, 0, -1])[k % 4]
        c = 1.0 / np.sqrt(n)
        if kind == "off":
            off = rng.random(n) < 1.0 / 3.0
            P[:, off] = 0
            Q[:, off] = 0
    else:
        P = rng.choice([-1, 1], size=(m, n))
        Q = rng.choice([-1, 1], size=(m, n))
        c = {"pmj1": 1.0, "pmj": 1.0 / np.sqrt(2.0 * n), "twin": 1.0 / 32.0}[kind]
        if kind == "twin":
            P[:2] = 1
            Q[:2] = 1
    return c * P.astype(np.float64) + 1j * (c * Q.astype(np.float64))


def int_vectors(rng, nv, k, bits=20):
    """Integer-valued complex vectors with |component| < 2^bits."""
    lim = 1 << bits
    return (rng.integers(-lim + 1, lim, (nv, k)) + 1j * rng.integers(-lim + 1, lim, (nv, k))).astype(np.complex128)


def rand_vectors(rng, nv, k, spread=8.0):
    """Full-mantissa complex vectors: unit normals with a per-vector scale over 2^+-spread."""
    s = np.exp2(rng.uniform(-spread, spread, (nv, 1)))
    return (rng.standard_normal((nv, k)) + 1j * rng.standard_normal((nv, k))) * s


def edge_vectors(rng, nv, k):
    """The exponent edges, one per vector in turn: max|v| an exact power of two; max|v| one ulp below a power
    of two; one component 2^40 times the rest; plain unit normals."""
    V = rand_vectors(rng, nv, k, spread=0.0)
    Vr = V.view(np.float64)
    for j in range(nv):
        kind = j % 4
        mx = np.max(np.abs(Vr[j]))
        if kind == 0:
            top = 2.0 ** (j % 7 - 3)
            Vr[j] *= 0.5 * top / mx
            Vr[j, np.argmax(np.abs(Vr[j]))] = top
        elif kind == 1:
            top = np.nextafter(2.0 ** (j % 5), 0.0)
            Vr[j] *= 0.5 * top / mx
            Vr[j, np.argmax(np.abs(Vr[j]))] = -top
        elif kind == 2:
            Vr[j, (3 * j) % Vr.shape[1]] = mx * 2.0 ** 40
    return V
