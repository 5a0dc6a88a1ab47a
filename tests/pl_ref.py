"""Restatements of the PhaseLift step kernels one launch at a time (csrc/ace_phaselift.hip through ace_pl_host;
tests/test_gpu_pl.py), in numpy with np.longdouble accumulation, each written from the TFOCS lines the kernel's
comment cites (tfocs_AT.m, tfocs_backtrack.m, tfocs_iterate.m, prox_trace.m, MyPhaseLift.m), not through
tfocs_oracle.tfocs_at_tracels (which stays the end-to-end oracle; tests/test_pl_ref.py chains these against it).

Every restatement takes the arrays of the entry by name (a dict ``A``), the state [batch][len(STATE)] and the
parameters, and returns ``(arrays, state, tol)``:
  arrays  name -> expected contents of every buffer the operation writes (np.longdouble / clongdouble where rounded,
          the input's own dtype where the result is a copy)
  state   the expected state (float64; fields with a tolerance hold the longdouble value rounded once)
  tol     name -> per-real-component bound (same shape as the array's float view), "state" -> [batch][len(STATE)];
          a name that is absent, or a zero, means bit exact.
Buffers that are not returned must come back as they went in (the entry's guard_ok, and test_gpu_pl's own check).

Tolerances (EPS = 2^-52, u = EPS / 2), none of them fitted to what the kernels return:
  copies, integer and flag state, single correctly rounded operations (a - b, L * alpha, L / beta, sqrt, a * s of a
          real scalar and a complex entry, 1 / x): bit exact -- IEEE gives one answer, with or without contraction;
  entry-wise combinations: c EPS sum |terms|, c the number of roundings between an input and the result in the
          kernel's expression written without FMA (contraction only removes roundings):
          make_y / set_Ay / make_x  om * u + th * w: c = 3;  prox_in  0.5 ((zo - st G)_ij + conj (zo - st G)_ji): c = 3;
          take_z  0.5 (u + conj l): c = 1, its side branch adds 0.5 (w1 + conj w2) - tau: c = 5 over all terms;
          assemble  P = v (sgn (lam - tau)): c = 2;  C_z = lambda * misc[1]: c = 1;
  reductions over N real terms: N EPS sum |t_i| (any summation order, product roundings included), plus the
          first-order propagation of the bounds of entries that were themselves rounded (x in make_x, g in grad /
          backtrack);
  scalars derived from them: the bound carried through the few operations that follow (stated at each place);
  3M GEMMs (gy, zasm, the GEMM of apply_a): linop_ref.gemm_tol;
  chol: |R^H R - K| <= gamma_{m+1} |R|^H |R| with gamma_k = 4 k u / (1 - 4 k u): Higham, Accuracy and Stability of
          Numerical Algorithms, Thm 10.3, with the real model's 2u per inner-product term (one multiply, one add)
          replaced by 4u for complex arithmetic (a complex multiply is within sqrt(2) gamma_2 < 3u, Lemma 3.5; one
          complex add u); the division by the pivot is one of the m + 1 factors.  gamma_k = 2 k EPS below.
  final_vec, reduced: |R w - s| <= gamma_d |R| |w| (Higham Thm 8.5 with the same complex constant; the kernel's
          multiplication by 1 / r_jj instead of a division adds one rounding to the diagonal factor, inside 4u).
"""
from __future__ import annotations

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
EPS = float(np.finfo(np.float64).eps)
STATE = ("L", "L_old", "theta", "theta_old", "f_x", "f_y", "C_x", "C_z", "cntr_Ax", "cntr_Ay", "xy_sq", "nx2", "ndx2",
         "dot_xy_g", "localL", "step", "n_iter", "restart_iter", "backtrack_simple", "backtrack_steps", "have_gAy",
         "have_gy", "have_gAx", "ycomp", "need_Ay", "need_Ax", "inner", "done", "status")
IX = {k: i for i, k in enumerate(STATE)}
PARAMS = dict(cntr_reset=50, restart=200, maxIts=4000, alpha=0.9, beta=0.5, Lexact=np.inf, tol=1e-10, L0=1.0,
              lam_reg=5e-2)
ACE_ST_CONVERGED = 1


def params(**kw):
    p = dict(PARAMS)
    p.update(kw)
    return p


def fv(x):
    """The float64 view of a complex128 array (re, im interleaved along the last axis); real arrays as they are."""
    x = np.ascontiguousarray(x)
    return x.view(np.float64) if x.dtype == np.complex128 else x


def fvl(x):
    """The same for longdouble / clongdouble values."""
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return np.stack([x.real, x.imag], axis=-1).reshape(x.shape[:-1] + (2 * x.shape[-1],)).astype(LD)
    return x.astype(LD)


def gamma(k):
    """gamma_k of the module docstring for complex arithmetic: 4 k u = 2 k EPS."""
    return 2.0 * k * EPS


class St:
    """Column access to a state array (a copy)."""

    def __init__(self, S):
        self.S = np.array(S, dtype=np.float64)
        self.T = np.zeros_like(self.S)

    def __getitem__(self, k):
        return self.S[:, IX[k]]

    def set(self, b, k, v, tol=0.0):
        self.S[b, IX[k]] = float(v)
        self.T[b, IX[k]] = float(tol)


def _om(th):
    """The double 1 - theta the kernels form."""
    return np.float64(1.0) - np.float64(th)


def _comb(om, u, th, w):
    """om * u + th * w per real component in longdouble and its c = 3 bound."""
    a, b = LD(om) * fvl(u), LD(th) * fvl(w)
    return a + b, 3 * EPS * (np.abs(a) + np.abs(b)).astype(np.float64)


def _as_c(v):
    """[.., 2k] longdouble reals -> [.., k] clongdouble."""
    return v[..., 0::2] + 1j * v[..., 1::2].astype(CLD)


# ------------------------------------------------------------------------------------------------ the operations
def init(A, S, p):
    """tfocs_initialize.m: x0 = 0 -> f_x = 0.5 ||b||^2, g_Ax = -b, y = z = x, theta = Inf, L = L0."""
    b = A["bvec"]
    B, m = b.shape
    s = St(np.zeros((B, len(STATE))))
    for i in range(B):
        t = b[i].astype(LD) ** 2
        f = 0.5 * t.sum()
        tl = 0.5 * m * EPS * float(t.sum())
        s.set(i, "L", p["L0"])
        s.set(i, "theta", np.inf)
        s.set(i, "f_x", f, tl)
        s.set(i, "f_y", f, tl)
        for k in ("backtrack_simple", "have_gAy", "have_gAx"):
            s.set(i, k, 1)
    return dict(gAy=-b, gAx=-b), s.S, dict(state=s.T)


def outer_begin(A, S, p):
    """tfocs_AT.m:22-31."""
    s = St(S)
    out = {k: np.array(A[k]) for k in ("xo", "zo", "Axo", "Azo")}
    for i in range(len(s.S)):
        if s["done"][i]:
            continue
        for dst, src in (("xo", "x"), ("zo", "z"), ("Axo", "Ax"), ("Azo", "Az")):
            out[dst][i] = A[src][i]
        s.set(i, "L_old", s["L"][i])
        s.set(i, "L", np.float64(s["L"][i]) * np.float64(p["alpha"]))
        s.set(i, "theta_old", s["theta"][i])
        s.set(i, "inner", 1)
    return out, s.S, {}


def theta_of(L, L_old, th_old):
    """tfocs_AT.m:35 in longdouble and its bound: seven roundings (L / L_old, theta_old^2, their quotient, 1 +, sqrt,
    1 +, 2 /), every intermediate positive and every stage of condition number <= 1: 7 EPS theta."""
    if np.isinf(th_old):
        return LD(1.0), 0.0   # 4 (L / L_old) / Inf = 0 exactly
    t = LD(2.0) / (1 + np.sqrt(1 + 4 * (LD(L) / LD(L_old)) / (LD(th_old) * LD(th_old))))
    return t, 7 * EPS * float(t)


def theta(A, S, p):
    """tfocs_AT.m:33-45 (theta, the A_y counter); act and the step's counters."""
    s = St(S)
    B = len(s.S)
    act = np.zeros(B, np.int32)
    cnt = np.array(A["cnt"])
    margins = []
    for i in range(B):
        if not s["inner"][i] or s["done"][i]:
            continue
        act[i] = 1
        t, tl = theta_of(s["L"][i], s["L_old"][i], s["theta_old"][i])
        if tl:   # (theta_old = Inf gives theta = 1 exactly: a tie, not a margin)
            margins.append(("theta < 1", abs(float(t) - 1.0), tl))
        s.set(i, "theta", t, tl)
        yc = float(t) < 1.0
        s.set(i, "ycomp", yc)
        s.set(i, "need_Ay", 0)
        if yc:
            if s["cntr_Ay"][i] >= p["cntr_reset"]:
                s.set(i, "need_Ay", 1)
                s.set(i, "cntr_Ay", 0.0)
            else:
                s.set(i, "cntr_Ay", s["cntr_Ay"][i] + 1.0)
            s.set(i, "f_y", np.inf)
            s.set(i, "have_gAy", 0)
            s.set(i, "have_gy", 0)
        cnt[0] += 1
        cnt[1] += int(s["need_Ay"][i])
        cnt[4] += int(not s["have_gy"][i])
    return dict(act=act, cnt=cnt), s.S, dict(state=s.T, margins=margins)


def make_y(A, S, p):
    """y = (1 - theta) x_old + theta z_old (tfocs_AT.m:38)."""
    s = St(S)
    y = fvl(A["y"])
    tol = np.zeros(y.shape)
    for i in range(len(s.S)):
        if A["act"][i] and s["ycomp"][i]:
            y[i], tol[i] = _comb(_om(s["theta"][i]), A["xo"][i], s["theta"][i], A["zo"][i])
    return dict(y=y), s.S, dict(y=tol)


def set_ay(A, S, p):
    """A_y = A(y) when the counter fired, else (1 - theta) A_x_old + theta A_z_old (tfocs_AT.m:39-44)."""
    s = St(S)
    Ay = fvl(A["Ay"])
    tol = np.zeros(Ay.shape)
    for i in range(len(s.S)):
        if A["act"][i] and s["ycomp"][i]:
            if s["need_Ay"][i]:
                Ay[i] = A["Aex"][i]
            else:
                Ay[i], tol[i] = _comb(_om(s["theta"][i]), A["Axo"][i], s["theta"][i], A["Azo"][i])
    return dict(Ay=Ay), s.S, dict(Ay=tol)


def grad(A, S, p):
    """smooth_quad at A_y - b (tfocs_AT.m:48-49); step = 1 / (theta L), tau = lambda step; Pg = R o g_Ay."""
    s = St(S)
    B, m = A["Ay"].shape
    gAy, Pg, tau = np.array(A["gAy"]), fvl(A["Pg"]), A["tau"].astype(LD)
    tP, tt = np.zeros(Pg.shape), np.zeros(B)
    R = A["R"]
    for i in range(B):
        if not A["act"][i]:
            continue
        if not s["have_gAy"][i]:
            gAy[i] = A["Ay"][i] - A["bvec"][i]   # one correctly rounded subtraction
            t = gAy[i].astype(LD) ** 2
            s.set(i, "f_y", 0.5 * t.sum(), 0.5 * m * EPS * float(t.sum()))
            s.set(i, "have_gAy", 1)
        if not s["have_gy"][i]:
            Pg[i] = fv(R * gAy[i][None, :]).astype(LD)   # one rounding per component: exact in f64
        s.set(i, "have_gy", 1)
        st = 1.0 / (LD(s["theta"][i]) * LD(s["L"][i]))
        s.set(i, "step", st, 2 * EPS * abs(float(st)))
        tau[i] = LD(p["lam_reg"]) * st
        tt[i] = 3 * EPS * abs(float(tau[i]))
    return dict(gAy=gAy, Pg=Pg, tau=tau), s.S, dict(Pg=tP, tau=tt, state=s.T)


def gemm_ref(Lm, V, conj):
    """C[r][i] = sum_k op(L)[i][k] V[r][k] in clongdouble."""
    Lc = np.conj(Lm) if conj else Lm
    return V.astype(CLD) @ Lc.astype(CLD).T


def gy(A, S, p):
    """g_y = A*(g_Ay) = R diag(g) R^H from Pg = R o g: G[b] = Pg[b] R^H."""
    from linop_ref import gemm_tol
    B = A["Pg"].shape[0]
    G = np.stack([gemm_ref(A["R"], A["Pg"][i], True) for i in range(B)])
    tol = np.stack([gemm_tol(np.conj(A["R"]), A["Pg"][i]) for i in range(B)])
    return dict(G=fvl(G)), np.array(S), dict(G=tol)


def _w(A, s, i):
    """W = z_old - step G per real component (two roundings) and sum |terms|."""
    a, b = fvl(A["zo"][i]), LD(s["step"][i]) * fvl(A["G"][i])
    return a - b, (np.abs(a) + np.abs(b)).astype(np.float64)


def _herm_half(w, mag):
    """0.5 (w + w^H) of a [d][2d] real view and the matching 0.5 (|.| + |.|^T)."""
    d = w.shape[0]
    re, im = w[:, 0::2], w[:, 1::2]
    out = np.empty_like(w)
    out[:, 0::2] = 0.5 * (re + re.T)
    out[:, 1::2] = 0.5 * (im - im.T)
    mg = np.empty((d, 2 * d))
    mg[:, 0::2] = 0.5 * (mag[:, 0::2] + mag[:, 0::2].T)
    mg[:, 1::2] = 0.5 * (mag[:, 1::2] + mag[:, 1::2].T)
    return out, mg


def prox_in(A, S, p):
    """prox_trace.m:88-92: C = (W + W^H) / 2, W = z_old - step g_y."""
    s = St(S)
    C = fvl(A["C"])
    tol = np.zeros(C.shape)
    for i in range(len(s.S)):
        if A["act"][i]:
            w, mag = _w(A, s, i)
            C[i], mg = _herm_half(w, mag)
            tol[i] = 3 * EPS * mg
    return dict(C=C), s.S, dict(C=tol)


def assemble(A, S, p):
    """prox_trace.m:140-147: P = V^T diag(s), VT = V^T, s = +-(lam - tau) for the kept q < k; the column tiles at or
    beyond 32 ceil(k / 32) are not written; C_z = lambda * misc[1]."""
    s = St(S)
    B, d, _ = A["V"].shape
    P, VT = fvl(A["P"]), np.array(A["VT"])
    tol = np.zeros(P.shape)
    for i in range(B):
        if not A["act"][i]:
            continue
        k = int(A["misc"][i, 0])
        sgn = -1.0 if A["misc"][i, 2] != 0.0 else 1.0
        kw = min(d, 32 * ((k + 31) // 32))
        vt = np.zeros((d, kw), np.complex128)
        vt[:, :k] = A["V"][i][:k, :].T
        sv, sm = np.zeros(kw, LD), np.zeros(kw)
        sv[:k] = sgn * (A["lam"][i, :k].astype(LD) - LD(A["tau"][i]))
        sm[:k] = np.abs(A["lam"][i, :k]) + abs(A["tau"][i])
        VT[i][:, :kw] = vt
        P[i][:, :2 * kw] = fvl(vt.astype(CLD) * sv[None, :])
        tol[i][:, :2 * kw] = 2 * EPS * np.abs(fv(vt)) * np.repeat(sm, 2)[None, :]
        cz = LD(p["lam_reg"]) * LD(A["misc"][i, 1])
        s.set(i, "C_z", cz, EPS * abs(float(cz)))
    return dict(P=P, VT=VT), s.S, dict(P=tol, state=s.T)


def zasm(A, S, p):
    """z = V(:, tt) diag(s) V(:, tt)^H as one GEMM over the kept q < k: Znew[b] = P[b][:, :k] VT[b][:, :k]^H."""
    from linop_ref import gemm_tol
    B, d, _ = A["P"].shape
    Z, tol = np.zeros((B, d, 2 * d), LD), np.zeros((B, d, 2 * d))
    for i in range(B):
        k = int(A["misc"][i, 0])
        if k:
            Z[i] = fvl(gemm_ref(A["VT"][i][:, :k], A["P"][i][:, :k], True))
            tol[i] = gemm_tol(np.conj(A["VT"][i][:, :k]), A["P"][i][:, :k])
    return dict(Znew=Z), np.array(S), dict(Znew=tol)


def take_z(A, S, p):
    """z = (Z + Z^H) / 2 (prox_trace.m:146); the complement side adds (W + W^H) / 2 - tau I."""
    s = St(S)
    z = fvl(A["z"])
    tol = np.zeros(z.shape)
    for i in range(len(s.S)):
        if not A["act"][i]:
            continue
        zn = fvl(A["Znew"][i])
        v, mg = _herm_half(zn, np.abs(zn).astype(np.float64))
        if A["misc"][i, 2] != 0.0:
            w, mag = _w(A, s, i)
            hw, mw = _herm_half(w, mag)
            d = v.shape[0]
            v = v + hw
            v[np.arange(d), 2 * np.arange(d)] -= LD(A["tau"][i])
            mg = mg + mw
            mg[np.arange(d), 2 * np.arange(d)] += abs(A["tau"][i])
            tol[i] = 5 * EPS * mg
        else:
            tol[i] = EPS * mg
        z[i] = v
    return dict(z=z), s.S, dict(z=tol)


def apply_a_T(A):
    """T = X R by the RT GEMM: T[b][r][i] = sum_k RT[i][k] X[b][r][k], and its 3M bound."""
    from linop_ref import gemm_tol
    B = A["x"].shape[0]
    T = np.stack([gemm_ref(A["RT"], A["x"][i], False) for i in range(B)])
    tol = np.stack([gemm_tol(A["RT"], A["x"][i]) for i in range(B)])
    return fvl(T), tol


def diagform(R, T, act, out):
    """a_i = Re sum_r conj(R[r][i]) T[r][i] (initializeLinopPR.m:58) on a given T: 2 d real terms per entry."""
    B, d, m = T.shape
    o, tol = out.astype(LD), np.zeros(out.shape)
    for i in range(B):
        if act[i]:
            t = np.abs(R.real).astype(LD) * np.abs(T[i].real) + np.abs(R.imag).astype(LD) * np.abs(T[i].imag)
            o[i] = (R.real.astype(LD) * T[i].real + R.imag.astype(LD) * T[i].imag).sum(axis=0)
            tol[i] = 2 * d * EPS * t.sum(axis=0).astype(np.float64)
    return o, tol


def make_x(A, S, p):
    """tfocs_AT.m:55-71 and the reductions of tfocs_backtrack.m / tfocs_iterate.m:
    ||x - y||^2, ||x||^2, <x - y, g_y>, ||x - x_old||^2."""
    s = St(S)
    B, d, _ = A["x"].shape
    x, Ax = fvl(A["x"]), fvl(A["Ax"])
    tx, tA = np.zeros(x.shape), np.zeros(Ax.shape)
    cnt = np.array(A["cnt"])
    N = 2 * d * d
    for i in range(B):
        if not A["act"][i]:
            continue
        one = not s["ycomp"][i]
        th = s["theta"][i]
        if one:
            xn, dxn = fvl(A["z"][i]), np.zeros((d, 2 * d))
        else:
            xn, dxn = _comb(_om(th), A["xo"][i], th, A["z"][i])
        x[i], tx[i] = xn, dxn
        y, xo, G = fvl(A["y"][i]), fvl(A["xo"][i]), fvl(A["G"][i])
        xy, dx = xn - y, xn - xo
        # each difference: the entry's own bound plus one rounding
        dxy = dxn + EPS * np.abs(xy).astype(np.float64)
        ddx = dxn + EPS * np.abs(dx).astype(np.float64)
        for name, val, tl in (
                ("xy_sq", (xy * xy).sum(), N * EPS * float((xy * xy).sum()) + 2 * float((np.abs(xy) * dxy).sum())),
                ("nx2", (xn * xn).sum(), N * EPS * float((xn * xn).sum()) + 2 * float((np.abs(xn) * dxn).sum())),
                ("dot_xy_g", (xy * G).sum(), N * EPS * float(np.abs(xy * G).sum()) + float((np.abs(G) * dxy).sum())),
                ("ndx2", (dx * dx).sum(), N * EPS * float((dx * dx).sum()) + 2 * float((np.abs(dx) * ddx).sum()))):
            s.set(i, name, val, tl)
        need = 0
        if one:
            s.set(i, "C_x", s["C_z"][i])
            Ax[i] = A["Az"][i]
        else:
            if s["cntr_Ax"][i] >= p["cntr_reset"]:
                s.set(i, "cntr_Ax", 0.0)
                need = 1
            else:
                s.set(i, "cntr_Ax", s["cntr_Ax"][i] + 1.0)
                Ax[i], tA[i] = _comb(_om(th), A["Axo"][i], th, A["Az"][i])
            s.set(i, "C_x", np.inf)
        s.set(i, "need_Ax", need)
        s.set(i, "f_x", np.inf)
        s.set(i, "have_gAx", 0)
        cnt[2] += need
    return dict(x=x, Ax=Ax, cnt=cnt), s.S, dict(x=tx, Ax=tA, state=s.T)


def set_ax(A, S, p):
    s = St(S)
    Ax = np.array(A["Ax"])
    for i in range(len(s.S)):
        if A["act"][i] and s["need_Ax"][i]:
            Ax[i] = A["Aex"][i]
    return dict(Ax=Ax), s.S, {}


def backtrack(A, S, p):
    """tfocs_backtrack.m.  ``margins`` lists (what, |distance to the decision's threshold|, bound on that distance's
    error) for every decision taken from a rounded quantity; exact ties are not listed."""
    s = St(S)
    B, m = A["Ax"].shape
    gAx = np.array(A["gAx"])
    margins = []
    for i in range(B):
        if not A["act"][i]:
            continue
        if s["xy_sq"][i] == 0.0:
            s.set(i, "localL", np.inf)
            s.set(i, "inner", 0)
            continue
        simple = bool(s["backtrack_simple"][i])
        L, xy_sq, f_y = s["L"][i], s["xy_sq"][i], s["f_y"][i]
        g = A["Ax"][i] - A["bvec"][i]          # one correctly rounded subtraction per entry
        gl = g.astype(LD)
        f_x = 0.5 * (gl * gl).sum()
        t_fx = 0.5 * m * EPS * float((gl * gl).sum())
        if s["xy_sq"][i] / s["nx2"][i] < EPS:
            s.set(i, "cntr_Ax", np.inf)
        s.set(i, "f_x", f_x, t_fx)
        if simple:
            # q_x: three roundings over exact state values; f_x - q_x one more; 2 . / xy_sq and L + two more
            terms = abs(f_y) + abs(s["dot_xy_g"][i]) + abs(0.5 * L * xy_sq)
            q_x = LD(f_y) + LD(s["dot_xy_g"][i]) + 0.5 * LD(L) * LD(xy_sq)
            diff = f_x - q_x
            t_diff = t_fx + 3 * EPS * terms + EPS * abs(float(diff))
            localL = LD(L) + 2 * max(diff, LD(0.0)) / LD(xy_sq)
            if localL > LD(np.finfo(np.float64).max):   # (the quotient overflows in f64)
                margins.append(("overflow", float(np.log2(localL)) - 1024.0, 1.0))
                localL = LD(np.inf)
            with np.errstate(over="ignore"):
                t_L = 2 * t_diff / xy_sq + 3 * EPS * abs(float(localL)) if diff > -t_diff else 0.0
            if float(diff) != 0.0 or t_diff != 0.0:
                margins.append(("f_x - q_x", abs(float(diff)), t_diff))
            rhs = 1e-10 * max(abs(float(f_x)), abs(f_y))
            margins.append(("backtrack_simple", abs(abs(f_y - float(f_x)) - rhs), 2 * t_fx + 2 * EPS * rhs))
            s.set(i, "backtrack_simple", abs(f_y - float(f_x)) >= rhs)
        else:
            gAx[i] = g
            f1 = A["Ax"][i].astype(LD) - A["Ay"][i].astype(LD)
            f2 = gl - A["gAy"][i].astype(LD)
            d1 = EPS * (np.abs(A["Ax"][i]) + np.abs(A["Ay"][i]))
            d2 = EPS * (np.abs(g) + np.abs(A["gAy"][i]))
            v1 = (f1 * f2).sum()
            t_v1 = m * EPS * float(np.abs(f1 * f2).sum()) + float((d1 * np.abs(f2) + d2 * np.abs(f1)).sum())
            s.set(i, "have_gAx", 1)
            localL = 2 * v1 / LD(xy_sq)
            t_L = 2 * t_v1 / xy_sq + EPS * abs(float(localL))
        s.set(i, "backtrack_steps", s["backtrack_steps"][i] + 1)
        s.set(i, "localL", localL, t_L)
        if not (np.isinf(localL) or (localL == LD(L) and t_L == 0.0)):
            margins.append(("localL <= L", abs(float(localL) - L), t_L))
        if float(localL) <= L or L >= p["Lexact"]:
            s.set(i, "inner", 0)
            continue
        Lb = np.float64(L) / np.float64(p["beta"])     # one correctly rounded division
        if np.isinf(localL):
            newL, t_n = min(p["Lexact"], Lb), 0.0
        else:
            if np.isfinite(p["Lexact"]):
                margins.append(("localL vs Lexact", abs(float(localL) - p["Lexact"]), t_L))
            # L = min(Lexact, localL); L = min(Lexact, max(localL, L / beta)) with that new L
            l1 = min(LD(p["Lexact"]), localL)
            t1 = t_L if l1 == localL else 0.0
            lb2 = l1 / LD(p["beta"])
            cand = max(localL, lb2)
            t_c = t_L if cand == localL else (t1 / p["beta"] + EPS * abs(float(lb2)))
            newL = min(LD(p["Lexact"]), cand)
            t_n = t_c if newL == cand else 0.0
        s.set(i, "L", newL, t_n)
    return dict(gAx=gAx), s.S, dict(state=s.T, margins=margins)


def iterate(A, S, p):
    """tfocs_iterate.m: stopping tests (stopCrit 1) and the periodic restart.  Every value the tests read is an exact
    state value and every operation on it (sqrt, one product, max) is correctly rounded: the double evaluation below
    is the kernel's, bit for bit."""
    s = St(S)
    out = {k: np.array(A[k]) for k in ("y", "z", "Ay", "Az", "gAy")}
    cnt = np.array(A["cnt"])
    for i in range(len(s.S)):
        if s["done"][i]:
            continue
        n_iter = int(s["n_iter"][i]) + 1
        s.set(i, "n_iter", n_iter)
        norm_x, norm_dx = np.sqrt(np.float64(s["nx2"][i])), np.sqrt(np.float64(s["ndx2"][i]))
        f_y = s["f_y"][i]
        stop = 0
        if f_y != f_y:
            stop = 1
        elif norm_dx == 0.0:
            stop = int(n_iter > 1)
        elif norm_dx < np.float64(p["tol"]) * max(norm_x, 1.0):
            stop = 2
        elif n_iter == p["maxIts"]:
            stop = 3
        elif s["backtrack_steps"][i] > 0 and s["xy_sq"][i] == 0.0:
            stop = 4
        if stop:
            s.set(i, "done", 1)
            s.set(i, "status", stop)
            cnt[8] += 1
            continue
        s.set(i, "backtrack_steps", 0)
        if n_iter - int(s["restart_iter"][i]) == p["restart"]:
            s.set(i, "restart_iter", n_iter)
            s.set(i, "backtrack_simple", 1)
            s.set(i, "theta", np.inf)
            s.set(i, "f_y", s["f_x"][i])
            s.set(i, "have_gAy", s["have_gAx"][i])
            s.set(i, "have_gy", 0)
            out["y"][i] = A["x"][i]
            out["z"][i] = A["x"][i]
            out["Ay"][i] = A["Ax"][i]
            out["Az"][i] = A["Ax"][i]
            out["gAy"][i] = A["gAx"][i]
    out["cnt"] = cnt
    return out, s.S, {}


def chol_check(K, R, ok):
    """The checks of the module docstring on a computed factor; returns the worst residual / bound."""
    m = K.shape[0]
    assert int(ok) == 1
    assert np.all(np.tril(R, -1) == 0), "entries below the diagonal"
    dg = np.diagonal(R)
    assert np.all(dg.imag == 0) and np.all(dg.real > 0), "diagonal not real positive"
    Rl = R.astype(CLD)
    res = np.abs(Rl.conj().T @ Rl - K.astype(CLD)).astype(np.float64)
    bound = gamma(m + 1) * (np.abs(R).T @ np.abs(R))
    # |.| of a complex entry against a bound on the modulus: the component-wise statement of Thm 10.3
    return float(np.max(res / bound))


def chol_expect_bad(R, ok):
    """A matrix that is not positive definite: ok = 0 and a finite output; nothing else is asserted about R."""
    assert int(ok) == 0
    assert np.isfinite(fv(np.asarray(R))).all()


def transpose(A, S, p):
    return dict(RT=np.ascontiguousarray(A["R"].T)), np.array(S), {}


def final_vec_s(A, reduced):
    """sig_d = sqrt(lam_max) u (MyPhaseLift.m:106-107): sqrt and one real-by-complex product, bit exact in f64."""
    lam = A["lam"][:, 0]
    if reduced:
        sl = np.sqrt(np.maximum(lam, 0.0))
        return A["V1"] * sl[:, None]
    sl = np.sqrt(np.abs(lam))
    v = A["V1"] * sl[:, None]
    im = (lam < 0.0)[:, None]
    return np.where(im, -v.imag + 1j * v.real, v)


def final_vec_check(A, w, reduced):
    """C = x and the vector: exact (non-reduced), or the back-substitution residual |R w - s| <= gamma_d |R| |w|;
    returns the worst residual / bound (0 where exact)."""
    s = final_vec_s(A, reduced)
    if not reduced:
        assert np.array_equal(fv(w), fv(s))
        return 0.0
    R = A["R"]
    d = R.shape[0]
    worst = 0.0
    for i in range(len(w)):
        res = np.abs(R.astype(CLD) @ w[i].astype(CLD) - s[i].astype(CLD)).astype(np.float64)
        bound = gamma(d) * (np.abs(R) @ np.abs(w[i]))
        if np.all(s[i] == 0):
            assert np.all(w[i] == 0)
            continue
        worst = max(worst, float(np.max(res / np.maximum(bound, np.finfo(float).tiny))))
    return worst


def outputs(A, S, p):
    s = St(S)
    conv = ((s["status"] == 1) | (s["status"] == 2)).astype(np.int32) * ACE_ST_CONVERGED
    return dict(iters=s["n_iter"].astype(np.int32), status=(A["status"] | conv).astype(np.int32)), s.S, {}


OPS = dict(init=init, outer_begin=outer_begin, theta=theta, make_y=make_y, set_ay=set_ay, grad=grad, gy=gy,
           prox_in=prox_in, assemble=assemble, zasm=zasm, take_z=take_z, make_x=make_x, set_ax=set_ax,
           backtrack=backtrack, iterate=iterate, transpose=transpose, outputs=outputs)
STATE_OPS = {"init", "outer_begin", "theta", "grad", "assemble", "make_x", "backtrack", "iterate"}


# ------------------------------------------------------------------------------------------------ the comparison
def same(a, b):
    """Bit-for-bit equality up to the sign of NaN: equal, or both NaN."""
    a, b = fv(np.asarray(a)), fv(np.asarray(b))
    return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))


def ratio(got, exp, tol):
    """max |got - exp| / tol over the entries with a bound; entries with tol == 0 must be equal (returns inf if not).
    exp is longdouble (rounded once where tol == 0)."""
    got, tol = fv(np.asarray(got)), np.asarray(tol, np.float64)
    exp = np.asarray(exp)
    exp = fvl(exp) if exp.dtype in (LD, CLD) else fv(exp).astype(LD)
    if got.shape != exp.shape:
        return np.inf
    fin = np.isfinite(exp)
    z = (tol == 0) | ~fin
    if not same(got[z], exp[z].astype(np.float64)):
        return np.inf
    if z.all():
        return 0.0
    err = np.abs(got[~z].astype(LD) - exp[~z]).astype(np.float64)
    if not np.all(np.isfinite(got[~z])):
        return np.inf
    return float(np.max(err / tol[~z]))


def compare(res_arr, res_state, exp_arr, exp_state, tol, inputs):
    """The comparison the GPU suite makes: worst err / tol over every returned buffer (exact ones: 0 or inf), every
    other buffer of ``inputs`` bit for bit as it went in.  res_arr: name -> array as the device left it."""
    worst = 0.0
    for k, e in exp_arr.items():
        t = tol.get(k)
        r = ratio(res_arr[k], e, np.zeros(fv(np.asarray(res_arr[k])).shape) if t is None else t)
        worst = max(worst, r)
    if exp_state is not None:
        t = tol.get("state")
        worst = max(worst, ratio(res_state, exp_state, np.zeros(np.shape(exp_state)) if t is None else t))
    for k, v in inputs.items():
        if k not in exp_arr and k in res_arr and not same(res_arr[k], v):
            return np.inf
    return worst


def margins_hold(margins, factor=4.0):
    """Every decision's distance to its threshold leaves room for another summation order: at least ``factor``
    times the bound on that distance's error."""
    return all(m[-2] > factor * m[-1] for m in margins)
