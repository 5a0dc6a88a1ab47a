"""References for the private code-image kernels one launch at a time (csrc/ace_private.hip through ace_pc_host;
tests/test_gpu_pc.py; self-tested on the CPU by tests/test_pc_ref.py).  Exact products, fma_ref, the digit model, the
int8 tolerance and g_reference come from tests/linop_ref.py.

Code images (written from the layout comments of ace_private.hip)
-----------------------------------------------------------------
An entry c j^k has code k.  With mt = ceil(m/16), nct = ceil(n/16), nb32 = ceil(m/32), per realisation:
  cR  [m][nct] dwords, code of column 16 wd + u at bits 2u (codes past n are 0).  Every dword is defined.
  cA  uint4 ((ct nkgA + kg) 16 + o) 2 + h, dword j: outputs are rows 16 ct + o (ct < mt), K-step ks = 8 kg + 2 j + p
      holds columns 16 ks + 8 h + u at bit code_shift(p, u) = 8 (u & 3) + 2 (2 p + (u >> 2)).  nkgA = ceil(nct/8).
      Every dword is defined; codes of rows past m and columns past n are 0.
  cH  the same index with ct over nct column tiles (output column 16 ct + o), nkgH = ceil(mt/8), K-step ks holding rows
      16 ks + 8 h + u.  pc_pack's block rb writes dword j = rb & 3 of group kg = rb >> 2, so a dword is defined iff
      4 kg + j < nb32 (all its bits: rows past m code 0; an output column past n gives the dword 0); the other dwords
      of the last group are never written and keep the 0xFF bytes the entry starts the buffer from.  pgk_kernel
      must not let them reach a product (its ks < nksH guards).

I + K (pc_k_kernel)
-------------------
K_il = c^2 ((n0 - n2) + j (n1 - n3)) from the exact counts n_d = #{k: (k_ik - k_lk) mod 4 = d}; c^2 = fl(c c).  The
imaginary part and the off-diagonal real part are one rounding, fl(c^2 k); the diagonal is fl(1 + fl(c^2 n)) or, where
the compiler contracts, fl(1 + c^2 n): ``kmat_candidates`` gives both through Fraction.

One pgk launch (``step_reference``) and its error scales (``compare_step``)
---------------------------------------------------------------------------
u = 2^-53.  a1(z) = |Re z| + |Im z|.  Every bound is per real component, first order, with the small constants
rounded up; the reference itself is evaluated with exact products or in longdouble (u_ld = 2^-64), 2^-11 of these.
  S = fma(-M, 1/mu, Y)         as the kernel forms it: fma_ref, exact.
  T (avok)   = S - AX          one f64 subtraction of known operands: exact (e_T = 0).
  T (cold)   = S - c A V       V = fma(-N, 1/mu, Z) (N = 0 under nzero), c A V through the digit model at the exponent
                               of vbound: e_T = i8_tol(A) + u |T|.
  g = G_eff T                  G_eff: the lower tiles read back, their conjugate transposes above, diagonal tiles as
                               stored.  Exact product; the kernel's fma chains and shuffles sum at most 2 mp + 16 real
                               terms: e_g = sum_k a1(G_ik) e_T,k + (2 mp + 16) u sum_k a1(G_ik) a1(T_k).
  AX' = (Y - M/mu) - g         M/mu rounded, two subtractions: e_ax = e_g + 4u (a1(Y) + a1(M)/mu + a1(g)).
  cc = AX' + M/mu, d = |cc|    e_cc = e_ax + 2u (a1(Y) + a1(M)/mu + a1(g)); d = 0 exactly: cc = 1, d = 1 (the guard).
  Y' = cc (B/d + mu)/(1 + mu)  = cc mu/(1 + mu) + (B/(1 + mu)) cc/|cc|; |d(cc/|cc|)| <= |dcc|/d, |dcc| <= sqrt2 e_cc:
                               e_y = 2 e_cc (mu + |B|/d)/(1 + mu) + 8u a1(Y').
  M' = M + mu (AX' - Y')       e_M = mu (e_ax + e_y) + 4u (a1(M) + mu (a1(AX') + a1(Y'))).
  sums of squares s = sum |v_i|^2 over m entries with |dv_i| <= sqrt2 e_i per entry:
                               e_s = sum (2 sqrt2 |v_i| e_i + 2 e_i^2) + (m + 16) u s
                               obj2 (v = |AX'| - B, e = sqrt2 e_ax + 2u (|AX'| + |B|)), nAX2 (e_ax), nY2 (e_y),
                               nJM2 (e_ax + e_y), dY2 (e_y + u a1(Y)).
  W = c A^H g                  digit model of the reference g at the exponent of max|g| + max e_g:
                               e_W = i8_tol(A^H) + c sum_i (e_g,i re + e_g,i im)  (every entry has one unit component).
  nAtY = |c A^H Y'|^2, dAtY = |c A^H (Y' - Y)|^2   digit models of Y' and dY with e_w as for W from e_y (dY: + u a1),
                               then the sum rule above over the 2n real outputs.
The opt_Y decision sqrt(obj2) < opt_obj is exact given obj2; ``decision`` reports the margin
|sqrt(obj2) - opt_obj| against e_obj / (2 sqrt(obj2)) so that a test can assert the decision is not a tie.

The Schur recursion's constant
------------------------------
``schur_inverse`` is the recursion of pc_inv_rec in numpy f64 (split h = 32 ((s/32)/2), unpivoted Gauss-Jordan on the
32 x 32 blocks).  Over ``inv_inputs`` (the GPU suite's matrices) its worst
    || g - g* ||_inf / (u kappa_inf || g* ||_inf)
is SCHUR_CPU = 270.8, reached by the integer rank-8 update 4 I + R R^H at 256 (kappa_inf 6.6e3); the next figures are
8.8 (the same kind at 224) and 5.0 (at 160), and every I + K of a codebook and every banded integer matrix stays below
0.5.  Forming F = B A^-1 and S = D - F B^H explicitly is not backward stable: where D is dominated by the low-rank
part, S comes out of a cancellation and the error grows with kappa of the blocks, not of H alone (LAPACK's pivoted
inverse of the same matrices stays below 0.1).  The figure moves with the summation order (235 with a blocked
product, 174 .. 281 over other draws of R), so the self-test asserts it within a factor of 1.5, and the recursion
here sums in index order with elementwise operations only.  The GPU is held to SCHUR_MULT times SCHUR_CPU: the 3M
GEMM's 2 (K + 4) u against a conventional product and the other summation order are a small factor.
"""
import math
from fractions import Fraction

import numpy as np

import linop_ref as LR
from linop_ref import U

LD, CLD = np.longdouble, np.clongdouble
STATE = ("mu", "opt_obj", "vbound", "obj2", "nAX2", "nY2", "nJM2", "dY2", "dAtY", "nAtY")
FLAGS = ("done", "avok", "nzero", "optysrc")
SI = {k: i for i, k in enumerate(STATE)}
FI = {k: i for i, k in enumerate(FLAGS)}
SUMS = STATE[3:]
SENTINEL = -7.25e77
SCHUR_CPU = 270.8    # measured worst err / (u kappa ||g*||) of schur_inverse over inv_inputs
SCHUR_MULT = 8.0
MODELS = ("G_unconjugated", "diag_twice", "tile_row_dropped", "slots_swapped", "lut_q_for_nq", "N_despite_nzero",
          "AX_despite_cold", "M_without_mu", "no_zero_guard", "optysrc_kept")
IMAGE_MODELS = ("p1_shifted", "h_swapped", "unwritten_zero")
KMAT_MODELS = ("n1_n3_exchanged", "diag_without_one")


# ---------------------------------------------------------------- dimensions, codes, images
def dims(m, n):
    mt, nct = (m + 15) // 16, (n + 15) // 16
    return dict(mt=mt, mp=16 * mt, mp32=32 * ((m + 31) // 32), nb32=(m + 31) // 32, ntile=mt * (mt + 1) // 2, nct=nct,
                nkgH=(mt + 7) // 8, nkgA=(nct + 7) // 8, nH=nct * ((mt + 7) // 8) * 128,
                nA=mt * ((nct + 7) // 8) * 128, nR=m * nct)


def phase_code(k, c):
    """A = c j^k with exact components (c, 0), (0, c), (-c, 0), (0, -c)."""
    k = np.asarray(k, np.int64) % 4
    return c * np.array([1.0, 0.0, -1.0, 0.0])[k] + 1j * (c * np.array([0.0, 1.0, 0.0, -1.0])[k])


def codes_of(A):
    """(c, k) of one phase-code matrix as pc_pack reads it (c from the first entry); None where it must flag."""
    A = np.asarray(A, np.complex128)
    c = max(abs(A[0, 0].real), abs(A[0, 0].imag))
    if not (c > 0 and c <= 1.7e308):
        return None
    k = np.full(A.shape, -1, np.int64)
    k[(A.imag == 0) & (A.real == c)] = 0
    k[(A.real == 0) & (A.imag == c)] = 1
    k[(A.imag == 0) & (A.real == -c)] = 2
    k[(A.real == 0) & (A.imag == -c)] = 3
    return None if (k < 0).any() else (float(c), k)


def code_shift(p, u):
    return 8 * (u & 3) + 2 * (2 * p + (u >> 2))


def _image(kpad, nout_t, nkg, rows_are_k, model=None):
    """One A / A^H image: kpad [out][in] codes zero-padded to 16 nout_t x 128 nkg."""
    ct, kg, o, h, j, p, u = np.meshgrid(np.arange(nout_t), np.arange(nkg), np.arange(16), np.arange(2), np.arange(4),
                                        np.arange(2), np.arange(8), indexing="ij")
    ks = 8 * kg + 2 * j + p
    hh = 1 - h if model == "h_swapped" else h
    uu = (u + 1) % 8 if (model == "p1_shifted" and rows_are_k) else u
    inp = 16 * ks + 8 * hh + np.where(p == 1, uu, u)
    val = kpad[16 * ct + o, inp].astype(np.uint64) << (8 * (u & 3) + 2 * (2 * p + (u >> 2))).astype(np.uint64)
    w = np.bitwise_or.reduce(np.bitwise_or.reduce(val, axis=6), axis=5)
    return w.astype(np.uint32).reshape(-1)


def encode(k, model=None):
    """The three images of one realisation's codes k [m][n]: dict cH, cA, cR (uint32) and maskH (the defined dwords of
    cH; every dword of cA and cR is defined).  Undefined dwords hold 0xFFFFFFFF."""
    k = np.asarray(k, np.int64)
    m, n = k.shape
    d = dims(m, n)
    R, Cc = 128 * max(d["nkgH"], 1), 128 * max(d["nkgA"], 1)
    kp = np.zeros((max(R, 16 * d["mt"]), max(Cc, 16 * d["nct"])), np.int64)
    kp[:m, :n] = k
    cA = _image(kp, d["mt"], d["nkgA"], False, model if model == "h_swapped" else None)
    cH = _image(np.ascontiguousarray(kp.T), d["nct"], d["nkgH"], True, model)
    kg, j = np.meshgrid(np.arange(d["nkgH"]), np.arange(4), indexing="ij")
    dfn = (4 * kg + j < d["nb32"])[None, :, None, None, :]
    maskH = np.broadcast_to(dfn, (d["nct"], d["nkgH"], 16, 2, 4)).reshape(-1).copy()
    cH = np.where(maskH, cH, np.uint32(0 if model == "unwritten_zero" else 0xFFFFFFFF)).astype(np.uint32)
    kr = kp[:m, :16 * d["nct"]].reshape(m, d["nct"], 16).astype(np.uint64)
    cR = np.bitwise_or.reduce(kr << (2 * np.arange(16, dtype=np.uint64)), axis=2).astype(np.uint32).reshape(-1)
    return dict(cH=cH, cA=cA, cR=cR, maskH=maskH)


def decode(img, m, n):
    """Codes [m][n] read back from each image: dict cH, cA, cR."""
    d = dims(m, n)
    out = {}
    cR = np.asarray(img["cR"], np.uint32).reshape(m, d["nct"])
    out["cR"] = ((cR[:, :, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).reshape(m, -1)[:, :n].astype(np.int64)
    for name, nt, nkg, tr in (("cA", d["mt"], d["nkgA"], False), ("cH", d["nct"], d["nkgH"], True)):
        w = np.asarray(img[name], np.uint32).reshape(nt, nkg, 16, 2, 4)
        no, ni = (n, m) if tr else (m, n)
        k = np.zeros((no, ni), np.int64)
        for o_ in range(no):
            for i_ in range(ni):
                ks, r = divmod(i_, 16)
                h, u_ = divmod(r, 8)
                kg, q = divmod(ks, 8)
                j, p = divmod(q, 2)
                k[o_, i_] = (int(w[o_ // 16, kg, o_ % 16, h, j]) >> code_shift(p, u_)) & 3
        out[name] = k.T if tr else k
    return out


def compare_images(got, k):
    """Names of the images of one realisation (got: dict cH, cA, cR of dwords) that differ from the encoder's: the
    defined dwords bit for bit, the others still 0xFF bytes."""
    ref = encode(k)
    return [nm for nm in ("cH", "cA", "cR") if not np.array_equal(np.asarray(got[nm], np.uint32).reshape(-1), ref[nm])]


# ---------------------------------------------------------------- I + K
def kmat_counts(k):
    """(kr, ki) integer arrays: K / c^2 = (n0 - n2) + j (n1 - n3) from the difference counts."""
    k = np.asarray(k, np.int64)
    oh = [(k == a).astype(np.float64) for a in range(4)]   # (counts below 2^53: the f64 products are exact)
    cnt = [sum(oh[a] @ oh[(a - q) % 4].T for a in range(4)).astype(np.int64) for q in range(4)]
    assert np.array_equal(sum(cnt), np.full((k.shape[0],) * 2, k.shape[1]))
    return cnt[0] - cnt[2], cnt[1] - cnt[3]


def kmat_candidates(k, c, model=None):
    """The two correctly rounded candidates of I + K in the setup's mp32 x mp32 frame (identity outside m)."""
    m, n = k.shape
    mp32 = dims(m, n)["mp32"]
    kr, ki = kmat_counts(k)
    if model == "n1_n3_exchanged":
        ki = -ki
    c2 = c * c
    re, im = c2 * kr.astype(np.float64), c2 * ki.astype(np.float64)
    one = 0.0 if model == "diag_without_one" else 1.0
    a, b = re.copy(), re.copy()
    for i in range(m):
        a[i, i] = one + re[i, i]
        b[i, i] = float(Fraction(one) + Fraction(c2) * int(kr[i, i]))
    out = []
    for x in (a, b):
        M = np.eye(mp32, dtype=np.complex128)
        M[:m, :m] = x + 1j * im
        out.append(M)
    return out


def kmat_matches(got, k, c):
    a, b = kmat_candidates(k, c)
    return bool(np.all(((got.real == a.real) | (got.real == b.real)) & (got.imag == a.imag)))


# ---------------------------------------------------------------- inverses
def _gj32(H):
    P = H.copy()
    s = P.shape[0]
    for p in range(s):
        pinv = 1.0 / P[p, p]
        row = P[p] * pinv
        row[p] = pinv
        col = P[:, p].copy()
        P[:, p] = 0.0
        P -= np.outer(col, row)
        P[p] = row
    return P


def _mm(a, b):
    """a b accumulated over the inner index in order, elementwise f64 operations only (no BLAS: the figure below
    must not depend on a library's blocking)."""
    acc = np.zeros((a.shape[0], b.shape[1]), np.complex128)
    for q in range(a.shape[1]):
        acc += a[:, q:q + 1] * b[q:q + 1, :]
    return acc


def schur_inverse(H):
    """pc_inv_rec in numpy f64."""
    H = np.array(H, np.complex128)
    s = H.shape[0]
    if s <= 32:
        return _gj32(H)
    h = 32 * ((s // 32) // 2)
    A, B, D = H[:h, :h], H[h:, :h], H[h:, h:]
    Ai = schur_inverse(A)
    F = _mm(B, Ai.conj().T)
    S = D - _mm(F, B.conj().T)
    Si = schur_inverse(S)
    T = _mm(F.conj().T, Si.conj().T)
    out = np.empty_like(H)
    out[:h, :h] = Ai + _mm(T, F)
    out[:h, h:] = -T
    out[h:, :h] = -T.conj().T
    out[h:, h:] = Si
    return out


INV_SIZES = (32, 64, 96, 160, 224, 256)


def codes(seed, m, n, twin=False):
    k = np.random.default_rng([seed, m, n]).integers(0, 4, (m, n))
    if twin and m > 1:
        k[1] = k[0]
    return k


def inv_inputs(mp32):
    """[(name, H [mp32][mp32], m)]: I + K of codebooks (m = mp32, and m = mp32 - 15 padded with the identity, with
    two identical rows) and two Hermitian positive definite integer matrices that are no I + K."""
    out = []
    for name, m, n, c, tw in (("ipk", mp32, 2 * mp32, 1.0 / math.sqrt(2 * mp32), False),
                              ("ipk-pad-twin", mp32 - 15, 100, 0.25, True)):
        H = kmat_candidates(codes(7, m, n, tw), c)[0]
        out.append((name, H, m))
    rng = np.random.default_rng([11, mp32])
    R = rng.integers(-3, 4, (mp32, 8)) + 1j * rng.integers(-3, 4, (mp32, 8))
    out.append(("int-lowrank", 4.0 * np.eye(mp32) + R @ R.conj().T, mp32))
    R = rng.integers(-2, 3, (mp32, mp32)) + 1j * rng.integers(-2, 3, (mp32, mp32))
    R = np.tril(R, 0) * (np.abs(np.subtract.outer(np.arange(mp32), np.arange(mp32))) <= 3)
    out.append(("int-band", (R + 9.0 * np.eye(mp32)) @ (R + 9.0 * np.eye(mp32)).conj().T, mp32))
    return out


def inv_vectors(H, seed=0):
    """(T [4][s], g* longdouble, kappa_inf): two norm-attaining and two random right-hand sides."""
    s = H.shape[0]
    K = H - np.eye(s)
    Binv = np.linalg.inv(H)
    rng = np.random.default_rng([seed, s])
    T = np.concatenate([LR.norm_attaining(Binv, 2), LR.rand_vectors(rng, 2, s, spread=4.0)])
    g, kappa, _ = LR.g_reference(K, T)
    return T, g, kappa


def inv_ratio(Ginv, T, gstar, kappa):
    """max over the vectors of || Ginv T - g* ||_inf / (u kappa_inf || g* ||_inf); the product in longdouble."""
    g = (np.asarray(Ginv).astype(CLD) @ np.asarray(T).astype(CLD).T).T
    err = np.max(np.abs(g - gstar), axis=1).astype(np.float64)
    return float(np.max(err / (U * kappa * np.max(np.abs(gstar), axis=1).astype(np.float64))))


# ---------------------------------------------------------------- tiles
def tiles_of(G, m):
    """pc_tiles: Gt [ntile][16][16] with Gt[I (I + 1) / 2 + K][c][r] = G[16 I + r][16 K + c], zero outside m."""
    mt = (m + 15) // 16
    Gp = np.zeros((16 * mt, 16 * mt), np.complex128)
    Gp[:m, :m] = np.asarray(G)[:m, :m]
    out = np.zeros((mt * (mt + 1) // 2, 16, 16), np.complex128)
    for I in range(mt):
        for K in range(I + 1):
            out[I * (I + 1) // 2 + K] = Gp[16 * I:16 * I + 16, 16 * K:16 * K + 16].T
    return out


def g_effective(Gt, m, model=None):
    """The m x m matrix pgk applies: lower tiles, their conjugate transposes above, diagonal tiles as stored."""
    mt = (m + 15) // 16
    G = np.zeros((16 * mt, 16 * mt), np.complex128)
    for I in range(mt):
        for K in range(I + 1):
            if model == "tile_row_dropped" and m <= 48 and I == mt - 1:
                continue
            blk = np.asarray(Gt[I * (I + 1) // 2 + K]).T
            G[16 * I:16 * I + 16, 16 * K:16 * K + 16] = blk * (2.0 if (model == "diag_twice" and I == K) else 1.0)
            if K < I:
                G[16 * K:16 * K + 16, 16 * I:16 * I + 16] = blk.T if model == "G_unconjugated" else blk.conj().T
    return G[:m, :m]


# ---------------------------------------------------------------- the digit products
def expansions(k):
    """(E_A [2m][2n], E_AH [2n][2m]) integer real expansions of j^k and of its conjugate transpose."""
    J = phase_code(k, 1.0)
    return LR.real_expand(J).astype(np.int64), LR.real_expand(J.conj().T).astype(np.int64)


def digit_product(Eint, scale, v, e):
    """linop_ref.digit_model for one real vector v, with the integer product in two exact int64 halves (the
    self-test holds it equal to digit_model)."""
    w = np.rint(np.ldexp(np.asarray(v, np.float64), 54 - int(e)))
    hi = np.floor(w * 2.0 ** -28)
    lo = w - hi * 2.0 ** 28
    Ei = np.asarray(Eint, np.int64)
    s = (Ei @ hi.astype(np.int64)).astype(object) * (1 << 28) + (Ei @ lo.astype(np.int64)).astype(object)
    return np.array([math.ldexp(float(x), int(e) - 54) * scale for x in s])


def _re(z):
    return np.ascontiguousarray(np.asarray(z, np.complex128)).view(np.float64)


def _a1(z):
    return np.abs(z.real) + np.abs(z.imag)


def _sumsq(v_abs, e, cnt):
    """(s, e_s) of the module docstring's sum rule; v_abs: |v_i| (longdouble), e: per-entry component bound."""
    s = np.sum(v_abs * v_abs)
    es = np.sum(2 * math.sqrt(2) * v_abs * e + 2 * e * e) + (cnt + 16) * U * s
    return s, es


# ---------------------------------------------------------------- one pgk launch
def step_reference(inp, b):
    """Reference outputs and error scales of realisation b (not done) of one launch.  inp: dict with k [B][m][n], c [B],
    Gt [B][ntile][16][16], B, Yo, M, AX, Z, N, state, flags, yn_id.  Returns dict name -> (value, tol); vectors as
    f64 interleaved components."""
    k, c = np.asarray(inp["k"][b]), float(inp["c"][b])
    m, n = k.shape
    mp = 16 * ((m + 15) // 16)
    mu = float(inp["state"][b][SI["mu"]])
    imu = 1.0 / mu
    fl = inp["flags"][b]
    EA, EAH = expansions(k)
    Yo, M, Bv = np.asarray(inp["Yo"][b], np.complex128), np.asarray(inp["M"][b], np.complex128), np.asarray(inp["B"][b])
    S = LR.fma_ref(M[None], [imu], Yo[None])[0]
    if fl[FI["avok"]]:
        T = S - np.asarray(inp["AX"][b], np.complex128)
        eT = np.zeros(2 * m)
    else:
        Nv = np.zeros(n, np.complex128) if fl[FI["nzero"]] else np.asarray(inp["N"][b], np.complex128)
        V = LR.fma_ref(Nv[None], [imu], np.asarray(inp["Z"][b], np.complex128)[None])[0]
        e = LR.kernel_exp([inp["state"][b][SI["vbound"]]])
        av = digit_product(EA, c, _re(V), e[0])
        T = (_re(S) - av).view(np.complex128)
        eT = LR.i8_tol(EA, c, e, av[None])[0] + U * np.abs(_re(T))
    G = g_effective(inp["Gt"][b], m)
    hi, lo = LR.exact_cmatvec(G, T[None])
    g = (hi[0].astype(LD) + lo[0].astype(LD))
    gc = g[0::2] + 1j * g[1::2]
    G1, T1 = _a1(G), _a1(T)
    eTc = np.maximum(eT[0::2], eT[1::2])
    eg = G1 @ (2 * eTc) + (2 * mp + 16) * U * (G1 @ T1)
    # Y-step in longdouble
    Yl, Ml, Bl = Yo.astype(CLD), M.astype(CLD), Bv.astype(LD)
    mim = Ml * LD(imu)
    ax = (Yl - mim) - gc
    cc = ax + mim
    dd = np.abs(cc)
    zero = dd == 0
    cc = np.where(zero, CLD(1.0), cc)
    dd = np.where(zero, LD(1.0), dd)
    y = cc * ((Bl / dd + mu) / (1 + LD(mu)))
    jv = ax - y
    Mn = Ml + LD(mu) * jv
    dy = y - Yl
    base = (_a1(Yo) + _a1(M) * imu + _a1(gc)).astype(np.float64)
    eax = eg + 4 * U * base
    ecc = eax + 2 * U * base
    ddf = dd.astype(np.float64)
    ey = 2 * ecc * (mu + np.abs(Bv) / ddf) / (1 + mu) + 8 * U * _a1(y).astype(np.float64)
    eM = mu * (eax + ey) + 4 * U * (_a1(M) + mu * (_a1(ax) + _a1(y)).astype(np.float64))
    out = {}

    def vec(name, z, e_):
        zz = np.empty(2 * m)
        zz[0::2], zz[1::2] = z.real.astype(np.float64), z.imag.astype(np.float64)
        out[name] = (zz, np.repeat(e_, 2))
    vec("AX", ax, eax)
    vec("Yn", y, ey)
    vec("M", Mn, eM)
    aax = np.abs(ax)
    out["obj2"] = _sumsq(np.abs(aax - Bl), math.sqrt(2) * eax + 2 * U * (aax + np.abs(Bl)).astype(np.float64), m)
    out["nAX2"] = _sumsq(aax, eax, m)
    out["nY2"] = _sumsq(np.abs(y), ey, m)
    out["nJM2"] = _sumsq(np.abs(jv), eax + ey, m)
    edy = ey + U * _a1(Yo)
    out["dY2"] = _sumsq(np.abs(dy), edy, m)
    # the A^H products of g, Y', dY
    res = {}
    for name, z, e_ in (("W", gc, eg), ("y", y, ey), ("dy", dy, edy)):
        zr = np.empty(2 * m)
        zr[0::2], zr[1::2] = z.real.astype(np.float64), z.imag.astype(np.float64)
        bound = np.max(np.abs(zr)) if m else 0.0
        ex = LR.kernel_exp([bound])
        ex_up = LR.kernel_exp([bound + float(np.max(e_))])
        w = digit_product(EAH, c, zr, ex[0])
        tol = LR.i8_tol(EAH, c, ex_up, w[None])[0] + c * 2 * float(np.sum(e_))
        res[name] = (w, tol)
    out["W"] = res["W"]
    for name, key in (("nAtY", "y"), ("dAtY", "dy")):
        w, tol = res[key]
        wl = np.abs(w.astype(LD))
        s = np.sum(wl * wl)
        out[name] = (s, np.sum(2 * wl * tol + tol * tol) + (2 * n + 16) * U * s)
    out = {k_: (v, np.asarray(t, np.float64)) for k_, (v, t) in out.items()}
    out["zero_guard"] = zero
    return out


def decision(ref, opt_obj):
    """(imp, margin): the opt_Y decision sqrt(obj2) < opt_obj on the reference and |sqrt(obj2) - opt_obj| in units of
    the error scale of sqrt(obj2) (inf for an infinite opt_obj)."""
    v, t = float(ref["obj2"][0]), float(ref["obj2"][1])
    so = math.sqrt(v)
    if not math.isfinite(opt_obj):
        return so < opt_obj, math.inf
    return so < opt_obj, abs(so - opt_obj) / max(t / (2 * so) if so > 0 else math.sqrt(t), 1e-300)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def compare_step(got, inp, sentinel=SENTINEL, refs=None):
    """Every comparison of one launch.  got: name -> array for AX, M, Yn, W, optY ([B][.] c128), B, Yo, Z, N (handed
    back), state [B][10], flags [B][4].  Returns (fails, worst): the failed checks as strings and the worst err / tol
    per output name."""
    fails, worst = [], {}
    nb = len(inp["k"])
    yn_id = int(inp["yn_id"])
    for nm in ("B", "Yo", "Z", "N"):
        if not same_bits(np.asarray(got[nm]), np.asarray(inp[nm], np.asarray(got[nm]).dtype)):
            fails.append(f"{nm} was written")
    for b in range(nb):
        fi, si = np.asarray(inp["flags"][b]), np.asarray(inp["state"][b])
        fo, so = np.asarray(got["flags"][b]), np.asarray(got["state"][b])
        yn_in = inp["Yn"][b] if inp.get("Yn") is not None else None
        oy_in = inp["optY"][b] if inp.get("optY") is not None else None
        if fi[FI["done"]]:
            for nm in ("AX", "M", "Yn", "optY"):
                want = inp[nm][b] if inp.get(nm) is not None else np.full_like(np.asarray(got[nm][b]), sentinel)
                if not same_bits(np.asarray(got[nm][b]), np.asarray(want, np.complex128)):
                    fails.append(f"[{b}] done, yet {nm} changed")
            if not (_re(got["W"][b]) == sentinel).all():
                fails.append(f"[{b}] done, yet W written")
            if not (same_bits(so, si.astype(np.float64)) and np.array_equal(fo, fi)):
                fails.append(f"[{b}] done, yet the control block changed")
            continue
        ref = refs[b] if refs is not None else step_reference(inp, b)
        for nm in ("AX", "M", "Yn", "W"):
            v, t = ref[nm]
            err = np.abs(_re(got[nm][b]).astype(LD) - v.astype(LD)).astype(np.float64)
            r = math.inf
            if np.isfinite(err).all():
                r = float(np.max(np.where(err == 0, 0.0, err / np.maximum(t, 1e-300))))
            worst[nm] = max(worst.get(nm, 0.0), r)
            if not r <= 1.0:
                fails.append(f"[{b}] {nm}: err/tol {r:.3g}")
        for nm in SUMS:
            v, t = ref[nm]
            err = float(abs(LD(so[SI[nm]]) - v))
            r = 0.0 if err == 0 else (err / float(t) if math.isfinite(err) and t > 0 else math.inf)
            worst[nm] = max(worst.get(nm, 0.0), r)
            if not r <= 1.0:
                fails.append(f"[{b}] {nm}: err/tol {r:.3g}")
        for nm in ("mu", "opt_obj", "vbound"):
            if not same_bits(so[SI[nm]:SI[nm] + 1], si[SI[nm]:SI[nm] + 1].astype(np.float64)):
                fails.append(f"[{b}] {nm} changed")
        if not np.array_equal(fo[:3], fi[:3]):
            fails.append(f"[{b}] done / avok / nzero changed")
        # opt_Y: the deferred copy of the old Yn, then this step's decision (on the kernel's own obj2)
        oys = int(fi[FI["optysrc"]])
        imp = math.sqrt(so[SI["obj2"]]) < si[SI["opt_obj"]] if so[SI["obj2"]] >= 0 else False
        rimp, margin = decision(ref, float(si[SI["opt_obj"]]))
        if imp != rimp:
            fails.append(f"[{b}] opt_Y decision {imp}, reference {rimp} (margin {margin:.3g})")
        blank = np.full(np.asarray(got["optY"][b]).shape, complex(sentinel, sentinel))
        want = np.asarray(oy_in, np.complex128) if oy_in is not None else blank
        if yn_id and oys == yn_id:
            want = np.asarray(yn_in, np.complex128) if yn_in is not None else blank
        if not yn_id and imp:
            want = np.asarray(got["Yn"][b])
        if not same_bits(np.asarray(got["optY"][b]), want):
            fails.append(f"[{b}] optY is not the expected copy")
        want_src = (yn_id if imp else (0 if oys == yn_id else oys)) if yn_id else oys
        if int(fo[FI["optysrc"]]) != want_src:
            fails.append(f"[{b}] optysrc {int(fo[FI['optysrc']])}, expected {want_src}")
    return fails, worst


# ---------------------------------------------------------------- f64 model of the kernel, with faults
def model_result(inp, model=None, sentinel=SENTINEL):
    """What a kernel computing in f64 would hand back for inp (the `got` of compare_step), optionally with one of
    MODELS wrong.  model = None must pass compare_step: the tolerances hold for a plain f64 evaluation."""
    nb = len(inp["k"])
    m, n = np.asarray(inp["k"][0]).shape
    yn_id = int(inp["yn_id"])

    def start(nm, cols):
        x = inp.get(nm)
        return np.array(x, np.complex128) if x is not None else np.full((nb, cols), complex(sentinel, sentinel))
    got = dict(AX=start("AX", m), M=start("M", m), Yn=start("Yn", m), optY=start("optY", m),
               W=np.full((nb, n), complex(sentinel, sentinel)), B=np.array(inp["B"], np.float64),
               Yo=np.array(inp["Yo"], np.complex128),
               Z=np.array(inp["Z"], np.complex128), N=np.array(inp["N"], np.complex128),
               state=np.array(inp["state"], np.float64), flags=np.array(inp["flags"], np.int32))
    for b in range(nb):
        fl, st = got["flags"][b], got["state"][b]
        if fl[FI["done"]]:
            continue
        k, c = np.asarray(inp["k"][b]), float(inp["c"][b])
        mu = st[SI["mu"]]
        imu = 1.0 / mu
        EA, EAH = expansions(k)
        Yo, M, Bv = got["Yo"][b], got["M"][b].copy(), got["B"][b]
        oys = int(fl[FI["optysrc"]])
        if yn_id and oys == yn_id:
            got["optY"][b] = got["Yn"][b]
        S = LR.fma_ref(M[None], [imu], Yo[None])[0]
        avok = fl[FI["avok"]] or model == "AX_despite_cold"
        if avok:
            T = S - got["AX"][b]
        else:
            Nv = np.zeros(n, np.complex128) if (fl[FI["nzero"]] and model != "N_despite_nzero") else got["N"][b]
            V = LR.fma_ref(Nv[None], [imu], got["Z"][b][None])[0]
            av = digit_product(EA, c, _re(V), LR.kernel_exp([st[SI["vbound"]]])[0])
            T = (_re(S) - av).view(np.complex128)
        g = g_effective(inp["Gt"][b], m, model) @ T
        mim = M * imu
        ax = (Yo - mim) - g
        cc = ax + mim
        dd = np.abs(cc)
        if model != "no_zero_guard":
            z = dd == 0
            cc, dd = np.where(z, 1.0 + 0j, cc), np.where(z, 1.0, dd)
        with np.errstate(all="ignore"):
            y = cc * ((Bv / dd + mu) / (1.0 + mu))
        jv = ax - y
        got["AX"][b] = ax
        got["M"][b] = M + (jv if model == "M_without_mu" else mu * jv)
        got["Yn"][b] = y
        dy = y - Yo
        st[SI["obj2"]] = np.sum((np.abs(ax) - Bv) ** 2)
        st[SI["nAX2"]], st[SI["nY2"]] = np.sum(np.abs(ax) ** 2), np.sum(np.abs(y) ** 2)
        st[SI["nJM2"]], st[SI["dY2"]] = np.sum(np.abs(jv) ** 2), np.sum(np.abs(dy) ** 2)
        imp = math.sqrt(st[SI["obj2"]]) < st[SI["opt_obj"]]
        if not yn_id and imp:
            got["optY"][b] = y
        if yn_id:
            fl[FI["optysrc"]] = yn_id if imp else ((oys if model == "optysrc_kept" else 0) if oys == yn_id else oys)
        prods = []
        for z in (g, y, dy):
            zr = _re(z)
            ex = LR.kernel_exp([np.max(np.abs(zr))])[0] if np.isfinite(zr).all() else 0
            E = EAH
            if model == "lut_q_for_nq":   # the imaginary outputs take +q x instead of -q x
                E = EAH.copy()
                E[1::2, 0::2] = -E[1::2, 0::2]
            prods.append(digit_product(E, c, np.nan_to_num(zr), ex))
        got["W"][b] = prods[0].view(np.complex128)
        ny, dyv = np.sum(prods[1] ** 2), np.sum(prods[2] ** 2)
        if model == "slots_swapped":
            ny, dyv = dyv, ny
        st[SI["nAtY"]], st[SI["dAtY"]] = ny, dyv
    return got


# ---------------------------------------------------------------- the suite's data
def step_inputs(m, n, nb, seed, *, avok=1, nzero=0, yn_id=0, own_g=True, opt_obj=math.inf, optysrc=0, done=()):
    """Floating-point inputs of one launch for nb realisations (everything but Gt, which a GPU test reads back and
    the self-test takes from ``cpu_gt``).  c differs per realisation: 1/sqrt(n), 16/sqrt(n), 1/4, ..."""
    rng = np.random.default_rng([seed, m, n, nb])
    cs = [1.0 / math.sqrt(n), 16.0 / math.sqrt(n), 0.25]
    k = np.stack([codes(seed + b, m, n, twin=(b == 1)) for b in range(nb)])
    c = np.array([cs[b % 3] for b in range(nb)])
    A = np.stack([phase_code(k[b], c[b]) for b in range(nb)])
    cplx = lambda r, q: rng.standard_normal((r, q)) + 1j * rng.standard_normal((r, q))
    mu = rng.uniform(0.5, 4.0, nb)
    Z, N = cplx(nb, n) / math.sqrt(n), 0.1 * cplx(nb, n) / math.sqrt(n)
    Nuse = np.zeros_like(N) if nzero else N
    V = np.stack([LR.fma_ref(Nuse[b][None], [1.0 / mu[b]], Z[b][None])[0] for b in range(nb)])
    state = np.zeros((nb, len(STATE)))
    state[:, SI["mu"]], state[:, SI["opt_obj"]] = mu, opt_obj
    state[:, SI["vbound"]] = LR.maxabs_rows(V)
    state[:, 3:] = rng.uniform(1.0, 2.0, (nb, 7))   # stale sums: every one must be overwritten
    flags = np.zeros((nb, len(FLAGS)), np.int32)
    flags[:, FI["avok"]], flags[:, FI["nzero"]], flags[:, FI["optysrc"]] = avok, nzero, optysrc
    for b in done:
        flags[b, FI["done"]] = 1
    inp = dict(k=k, c=c, A=A, B=np.abs(rng.standard_normal((nb, m))) + 0.1, Yo=cplx(nb, m), M=0.3 * cplx(nb, m),
               AX=cplx(nb, m), Yn=cplx(nb, m), optY=cplx(nb, m), Z=Z, N=N, state=state, flags=flags, yn_id=yn_id,
               G=None)
    if nzero:   # the stored N of such a realisation is never read: poison it
        inp["N"] = np.full((nb, n), np.nan + 1j * np.nan)
    if not own_g:
        Gs = []
        for b in range(nb):
            R = cplx(m, m) / math.sqrt(m)
            Gs.append(np.linalg.inv(np.eye(m) + R @ R.conj().T))
        inp["G"] = np.stack(Gs)
    return inp


def cpu_gt(inp):
    """Gt as the setup would leave it, from a numpy inverse (self-test only)."""
    nb = len(inp["k"])
    m = np.asarray(inp["k"][0]).shape[0]
    out = []
    for b in range(nb):
        if inp.get("G") is not None:
            G = inp["G"][b]
        else:
            H = kmat_candidates(np.asarray(inp["k"][b]), float(inp["c"][b]))[0][:m, :m]
            G = np.linalg.inv(H)
        out.append(tiles_of(G, m))
    return np.stack(out)


def int_step_inputs(m, n, nb, seed):
    """Integer data: a caller-given integer Hermitian G (NaN in its strictly upper tiles), integer Yo / AX, M = 0,
    mu = 1, avok = 1, so that T = Yo - AX and g = G T are exact; returns (inp, AX_expected)."""
    rng = np.random.default_rng([seed, m, n, 77])
    inp = step_inputs(m, n, nb, seed, avok=1)
    gi = lambda r, q, lim: (rng.integers(-lim, lim + 1, (r, q)) + 1j * rng.integers(-lim, lim + 1, (r, q)))
    Gs, want = [], []
    inp["Yo"], inp["AX"] = gi(nb, m, 1000).astype(np.complex128), gi(nb, m, 1000).astype(np.complex128)
    inp["M"] = np.zeros((nb, m), np.complex128)
    inp["state"][:, SI["mu"]] = 1.0
    for b in range(nb):
        R = gi(m, m, 50)
        G = np.tril(R, -1) + np.tril(R, -1).conj().T + np.diag(rng.integers(1, 100, m)).astype(np.complex128)
        T = inp["Yo"][b] - inp["AX"][b]
        want.append(inp["Yo"][b] - G @ T)   # |entries| < 256 * 2 * 50 * 2 * 2000 < 2^53: exact in f64
        Gn = G.copy()
        ti = np.arange(m) // 16
        Gn[ti[:, None] < ti[None, :]] = np.nan + 1j * np.nan
        Gs.append(Gn)
    inp["G"] = np.stack(Gs)
    return inp, np.stack(want)
