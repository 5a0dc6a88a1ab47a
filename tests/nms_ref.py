"""References, inputs and derived tolerances for the A2nuclear m-space iteration kernel (csrc/ace_nucmsp.hip;
tests/test_gpu_nms.py, self-tested on the CPU by tests/test_nms_ref.py).  Nothing here calls project code.

(a) n-space truth
-----------------
``nspace_chain`` is InferADMM of inferLowRank_Nuclear.m at r = 1 on a genuine small problem: V = Z - N/mu, ArgMinX in
Woodbury form (X = V + A^H G ((Y - M/mu) - A V), G = (I + A A^H)^-1 the exact inverse), ArgMinY with its zero guard,
ArgMinZ = Shrink of the one singular value ||X + N/mu||, the M and N updates, the best-objective bookkeeping, the
residuals, the thresholds, the stop test and the mu update.  The stop test is in its lazy form: (P and D) or C is
decided at once (the dual part from ||A^H Y||, ||A^H (Y - Y0)|| in n-space), and an iteration with P and not C is
reported as pending, with the quantities the m-space kernel keeps for it.  Every iterate is a genuine n-vector; next
to it the chain books the coordinates the kernel uses (E = alpha X_init + A^H e), which it never reads back, so a
state of the chain converts to the kernel's inputs (``NChain.mspace``).  The arithmetic is a parameter: mpmath at
``zprox_ref.DPS`` digits (the algebra of DESIGN section 2.9 is checked against it) or numpy longdouble (the same
function, vectorised: the shapes of the GPU suite).

(b) m-space specification
-------------------------
``mspace_step`` evaluates the recurrences of the header comment of ace_nucmsp.hip on exactly the f64 inputs the kernel
gets -- the supplied A E_prev, ||E_prev||^2 and G are taken as given, K g := T - g -- in longdouble (or mpmath, or
plain f64: the same function).  For every output it returns the value and an absolute error scale S = kappa |value|:
  products          S_g[i] = sum_k |G_ik| S_T[k],  S_T = |Y| + |M|/mu + |c_v| |A E_prev|  (>= sum |G_ik| |T_k|)
  Y-step            first-order propagation of S_g through AX, C = AX + M/mu, Y' = C f, M'
  sums              sum of (2 |term| S_term + |term|^2)
  quadratic forms   sum of |terms| with the scales of the coefficients, <E_prev, A^H g> and ||A^H g||^2 propagated
  res_comb, pd_*, nep2'   the same, propagated through the square roots
so kappa = S / |value| is sum |terms| / |value| for a quadratic form and grows without bound where it cancels.

Tolerance: TOL_MULT u S with u = 2^-53.  TOL_MULT is not chosen by looking at the kernel: tests/test_nms_ref.py
measures the largest err / (u S) that the plain f64 transcription (``mspace_step(..., ar=F64)``) reaches on the
suite's inputs, asserts that it stays below ORACLE_RATIO, and the kernel gets 8 x ORACLE_RATIO (another summation
order, the 3M complex product, fused multiply-adds): the margin zprox_ref gives its kernels.
"""
import functools
import types
from dataclasses import dataclass, field

import mpmath as mp
import numpy as np

DPS = 40             # mpmath digits (the Z-step reference's, tests/zprox_ref.py)

U = 2.0 ** -53
# largest err / (u S) of the f64 transcription over the suite's inputs, rounded up
# (measured 3.662 at m121-n16-b17-k0, En; tests/test_nms_ref.py::test_oracle_ratio prints it), and the kernel's
# multiplier
ORACLE_RATIO = 3.7
TOL_MULT = 8.0 * ORACLE_RATIO
# largest deviation of the f64 transcription, chained from init, from the n-space truth over the chains of the GPU
# suite, relative (tests/test_nms_ref.py::test_chain_deviation prints the measured figures); the kernel gets 8 x
CHAIN_DEV = {"y": 1.8e-15, "x": 1.0e-15, "scal": 1.1e-14}
CHAIN_MULT = 8.0

STATE = ("mu", "last_res", "opt_obj", "na", "naz", "nbeta", "nep2", "nopt_a", "ncur_a", "pd_dZ2", "pd_nZ2", "pd_rc",
         "obj2", "nAX2", "nY2", "nJM2", "dY2", "dAtY", "nAtY", "nx0")
FLAGS = ("iters", "done", "status", "dpend")
ST_CONVERGED = 1
MODELS = ("G_transposed", "cv_times_mu", "stale_mu", "AE_without_Kg", "hp1_nE2", "hp1_nX2", "hp1_jn2", "hp1_dZ2",
          "dY2_wrong_buffer", "optW_az", "pad_in_sums", "swap_jl4")


# ---------------------------------------------------------------- arithmetic
class Arith:
    """The operations the references use, over numpy arrays of longdouble ('ld'), float64 ('f64') or mpmath numbers
    ('mp', object arrays)."""

    def __init__(self, kind):
        self.kind = kind
        self.obj = kind == "mp"
        self.inf = mp.inf if self.obj else np.inf
        if self.obj:
            self._re = np.frompyfunc(lambda z: mp.mpf(z.real), 1, 1)
            self._im = np.frompyfunc(lambda z: mp.mpf(z.imag), 1, 1)
            self._sqrt = np.frompyfunc(lambda v: mp.sqrt(v), 1, 1)
            self._f0 = np.frompyfunc(lambda v: v if v > 0 else mp.mpf(0), 1, 1)
            self._mpf = np.frompyfunc(lambda v: mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v, 1, 1)
            self._mpc = np.frompyfunc(lambda v: v if isinstance(v, (mp.mpc, mp.mpf)) else
                                      mp.mpc(float(np.real(v)), float(np.imag(v))), 1, 1)

    def r(self, x):
        if self.obj:
            x = np.asarray(x)
            return self._mpf(x.astype(object)) if x.size else x.astype(object)
        return np.array(x, dtype=np.longdouble if self.kind == "ld" else np.float64)

    def c(self, x):
        if self.obj:
            x = np.asarray(x)
            return self._mpc(x.astype(object)) if x.size else x.astype(object)
        return np.array(x, dtype=np.clongdouble if self.kind == "ld" else np.complex128)

    def re(self, z):
        return self._re(z) if self.obj else np.real(z)

    def im(self, z):
        return self._im(z) if self.obj else np.imag(z)

    def conj(self, z):
        return np.frompyfunc(lambda v: v.conjugate(), 1, 1)(z) if self.obj else np.conj(z)

    def abs2(self, z):
        a, b = self.re(z), self.im(z)
        return a * a + b * b

    def sqrt(self, x):
        return self._sqrt(x) if self.obj else np.sqrt(x)

    def cabs(self, z):
        return self.sqrt(self.abs2(z))

    def fmax0(self, x):
        """C's fmax(0, x): a NaN gives 0."""
        return self._f0(x) if self.obj else np.fmax(x, 0)

    def fmax(self, a, b):
        return np.maximum(a, b) if self.obj else np.fmax(a, b)

    def f64(self, x):
        """Round to f64 (complex or real)."""
        x = np.asarray(x)
        if x.dtype == object:
            flat = [complex(v) if isinstance(v, mp.mpc) else float(v) for v in x.ravel()]
            return np.array(flat).reshape(x.shape)
        return x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)


LD, F64, MP = Arith("ld"), Arith("f64"), Arith("mp")


def _where(mask, a, b):
    return np.where(mask, a, b)


def _rowsum(x):
    return np.sum(x, axis=1) if x.shape[1] else np.zeros(x.shape[0], dtype=x.dtype) * 0


def _quad(ar, v, K):
    """Re(v^H K v) per row and its scale sum_i |v_i| (|K| |v|)_i."""
    Kv = v @ K.T
    return ar.re(_rowsum(ar.conj(v) * Kv)), Kv


# ---------------------------------------------------------------- the Y-step, a function of its own
def ystep(ar, yo, M, B, g, mu, s_g=None, yo_d=None):
    """ArgMinY with its zero guard and the M update on AX = (Y - M/mu) - g, as the m-space kernels form it:
    returns Y', M', the five sums (obj2, nAX2, nY2, nJM2, dY2) and, with s_g (the scale of g), their scales.
    mu: [b]; the vectors [b][m].  yo_d: the Y that dY2 is taken against (yo)."""
    mu_ = mu[:, None]
    imu = 1 / mu_
    mi = M * imu
    ax = (yo - mi) - g
    cc = ax + mi
    d = ar.cabs(cc)
    z = d == 0
    cc = _where(z, cc * 0 + 1, cc)
    d = _where(z, d * 0 + 1, d)
    f = (B / d + mu_) / (1 + mu_)
    y = cc * f
    jv = ax - y
    Mn = M + jv * mu_
    aax = ar.cabs(ax) - B
    dy = y - (yo if yo_d is None else yo_d)
    sums = dict(obj2=_rowsum(aax * aax), nAX2=_rowsum(ar.abs2(ax)), nY2=_rowsum(ar.abs2(y)),
                nJM2=_rowsum(ar.abs2(jv)), dY2=_rowsum(ar.abs2(dy)))
    out = dict(Y=y, M=Mn, ax=ax, **sums)
    if s_g is not None:
        a_yo, a_mi, a_ax, a_y = ar.cabs(yo), ar.cabs(mi), ar.cabs(ax), ar.cabs(y)
        s_ax = a_yo + a_mi + s_g
        s_cc = s_ax + a_mi
        s_y = 2 * abs(f) * s_cc + a_y
        s_jv = s_ax + s_y
        a_jv, a_dy = ar.cabs(jv), ar.cabs(dy)
        s_dy = s_y + a_yo
        out["scale"] = dict(
            Y=s_y, M=ar.cabs(M) + mu_ * s_jv,
            obj2=_rowsum(2 * abs(aax) * (s_ax + a_ax + abs(B)) + aax * aax),
            nAX2=_rowsum(2 * a_ax * s_ax + a_ax * a_ax), nY2=_rowsum(2 * a_y * s_y + a_y * a_y),
            nJM2=_rowsum(2 * a_jv * s_jv + a_jv * a_jv), dY2=_rowsum(2 * a_dy * s_dy + a_dy * a_dy))
    return out


# ---------------------------------------------------------------- (b) the m-space specification
def _pad_rows(x, mp_):
    """Entries m .. mp-1 of each row as a kernel that forgot `i < m` would read them: the flat continuation."""
    b, m = x.shape
    idx = np.minimum(np.arange(b)[:, None] * m + np.arange(m, mp_)[None, :], b * m - 1)
    return x.reshape(-1)[idx]


def mspace_step(inp, ar=LD, model=None, fin=False):
    """One launch of the iteration kernel (fin: only the pending tests) on the inputs ``inp`` (a dict: G, K [m][m];
    B, Yo, Yn, M, Eo, AEo [b][m]; state [b][len(STATE)], flags [b][len(FLAGS)]; n, it, tol_rel, tol_abs, rho,
    fixed_iters, done_count).  Returns a dict: ``val`` (every output, in ar's numbers), ``scale`` (absolute error
    scales, same keys where defined), ``state`` / ``flags`` (the control block after the launch), ``done_count``,
    ``mask`` (live, pend_in, stop_in, run, imp, cur, pendn, conv, stop, bump, bump_in, dual_pass) and ``margin``
    (relative distance of every evaluated decision from a tie; NaN where it is not evaluated).
    model: one of MODELS, a wrong step (for the separation test)."""
    G, K = ar.c(inp["G"]), ar.c(inp["K"])
    if model == "G_transposed":
        G = G.T
    Yo, M, Eo, AEo = ar.c(inp["Yo"]), ar.c(inp["M"]), ar.c(inp["Eo"]), ar.c(inp["AEo"])
    Yn_in = ar.c(inp["Yn"]) if inp.get("Yn") is not None else Yo * 0
    B = ar.r(inp["B"])
    b, m = Yo.shape
    n, it = int(inp["n"]), int(inp["it"])
    tol_rel, tol_abs, rho = (ar.r(inp[k]) for k in ("tol_rel", "tol_abs", "rho"))
    fixed = bool(inp["fixed_iters"])
    st = np.asarray(inp["state"])
    S = {k: ar.r(st[:, i]) for i, k in enumerate(STATE)}
    fl = np.asarray(inp["flags"]).astype(np.int64)
    F = {k: fl[:, i].copy() for i, k in enumerate(FLAGS)}
    done_count = int(inp.get("done_count", 0))
    val, scale, margin, mask = {}, {}, {}, {}
    nanr = np.full(b, np.nan)

    def rel(a_, b_):
        a64, b64 = ar.f64(a_).astype(np.float64), ar.f64(b_).astype(np.float64)
        with np.errstate(all="ignore"):
            d = np.abs(a64 - b64) / np.maximum(np.abs(a64), np.abs(b64))
        return np.where(np.isinf(a64) | np.isinf(b64), np.inf, d)

    live = F["done"] == 0
    pend = live & (F["dpend"] != 0)
    mu_entry = S["mu"].copy()
    mask["live"], mask["pend_in"] = live.copy(), pend.copy()
    stop_in, bump_in, dpass = np.zeros(b, bool), np.zeros(b, bool), np.zeros(b, bool)
    margin["dual"], margin["bump_in"] = nanr.copy(), nanr.copy()
    # ---- the pending convergence tests of the previous iteration (dual_finish)
    if pend.any():
        v1 = Yo - Yn_in
        nv, Kv0 = _quad(ar, Yo, K)
        dv, Kv1 = _quad(ar, v1, K)
        aK = ar.cabs(K)
        a0, a1 = ar.cabs(Yo), ar.cabs(v1)
        s1 = a0 + ar.cabs(Yn_in)
        s_nv = 2 * _rowsum(a0 * (a0 @ aK.T))
        s_dv = _rowsum(s1 * ar.cabs(Kv1) + a1 * (s1 @ aK.T))
        mu = S["mu"]
        rd = mu * ar.sqrt(ar.fmax0(dv) + S["pd_dZ2"])
        td = tol_abs * ar.sqrt(ar.r(2 * n)) + tol_rel * ar.sqrt(ar.fmax0(nv) + S["pd_nZ2"])
        dpass = pend & np.asarray(rd < td, bool)
        stop_in = dpass & (not fixed)
        cont = pend & ~stop_in
        bump_in = cont & np.asarray(S["pd_rc"] > S["last_res"] * ar.r(0.9), bool)
        margin["dual"] = np.where(pend, rel(rd, td), np.nan)
        margin["bump_in"] = np.where(cont, rel(S["pd_rc"], S["last_res"] * ar.r(0.9)), np.nan)
        S["dAtY"], S["nAtY"] = _where(pend, dv, S["dAtY"]), _where(pend, nv, S["nAtY"])
        scale["dAtY"], scale["nAtY"] = s_dv, s_nv
        scale["res_dual"] = mu * (s_dv / (2 * ar.sqrt(ar.fmax0(dv) + S["pd_dZ2"]) + ar.r(1e-300))) + rd
        val["res_dual"], val["t_dual"] = rd, td
        F["dpend"] = np.where(pend, 0, F["dpend"])
        F["status"] = np.where(dpass, F["status"] | ST_CONVERGED, F["status"])
        F["done"] = np.where(stop_in, 1, F["done"])
        done_count += int(stop_in.sum())
        S["mu"] = _where(bump_in, mu * rho, mu)
        S["last_res"] = _where(cont, S["pd_rc"], S["last_res"])
    mask.update(stop_in=stop_in, bump_in=bump_in, dual_pass=dpass)
    run = live & ~stop_in
    mask["run"] = run
    for k in ("imp", "cur", "pendn", "conv", "stop", "bump", "shrunk0"):
        mask[k] = np.zeros(b, bool)
    if fin:
        return dict(val=val, scale=scale, state=S, flags=F, done_count=done_count, mask=mask, margin=margin)

    # ---- T, g = G T
    mu = S["mu"]
    muT = mu_entry if model == "stale_mu" else mu
    az, an, al, ne = S["naz"], S["nbeta"], S["na"], S["nep2"]
    cv = az - an * mu if model == "cv_times_mu" else az - an / mu
    cvT = az - an * muT if model == "cv_times_mu" else az - an / muT
    T = (Yo - M / muT[:, None]) - cvT[:, None] * AEo
    g = T @ G.T
    if model == "swap_jl4":
        perm = np.arange(b)
        for j in range(b):
            jl = j % 16
            o = j + 4 if (jl // 4) % 2 == 0 else j - 4
            if 0 <= o < b:
                perm[j] = o
        g = g[perm]
    s_T = ar.cabs(Yo) + ar.cabs(M) / mu[:, None] + abs(cv)[:, None] * ar.cabs(AEo)
    s_g = s_T @ ar.cabs(G).T
    # ---- the Y-step and the sums
    ys = ystep(ar, Yo, M, B, g, mu, s_g, yo_d=Yn_in if model == "dY2_wrong_buffer" else None)
    kg = T - g
    En = az[:, None] * Eo + g
    AEn = az[:, None] * AEo + (kg if model != "AE_without_Kg" else 0)
    hp = ar.re(_rowsum(ar.conj(AEo) * g))
    hh_raw = ar.re(_rowsum(ar.conj(g) * kg))
    sums = {k: ys[k] for k in ("obj2", "nAX2", "nY2", "nJM2", "dY2")}
    mp_ = (m + 31) & ~31
    if model == "pad_in_sums" and mp_ > m:
        pz = _pad_rows(Yo, mp_) * 0
        yp = ystep(ar, _pad_rows(Yo, mp_), _pad_rows(M, mp_), _pad_rows(B, mp_), pz, mu)
        for k in sums:
            sums[k] = sums[k] + yp[k]
    hh = ar.fmax0(hh_raw)
    a_g, a_ae, a_kg = ar.cabs(g), ar.cabs(AEo), ar.cabs(kg)
    s_hp = _rowsum(a_ae * (s_g + a_g))
    s_hh = _rowsum(s_g * a_kg + a_g * (s_T + s_g) + a_g * a_kg)
    # ---- the Z-step of each realisation: prox, residual norms
    c2 = {k: (1 if model == "hp1_" + k else 2) for k in ("nE2", "nX2", "jn2", "dZ2")}
    imu = 1 / mu
    nE2 = ar.fmax0(az * az * ne + c2["nE2"] * az * hp + hh)
    s_nE2 = az * az * ne + 2 * abs(az) * s_hp + s_hh
    nE = ar.sqrt(nE2)
    pos = np.asarray(nE > 0, bool)
    nEs = _where(pos, nE, nE * 0 + 1)
    s = _where(pos, ar.fmax0(nE - imu) / nEs, nE * 0)
    s_nE = _where(pos, s_nE2 / (2 * nEs), ar.sqrt(s_nE2)) + nE
    shr0 = ~np.asarray(nE > imu, bool)
    s_s = _where(shr0, nE * 0, (imu / nEs) * (s_nE / nEs) + 1)
    s_cv = abs(az) + abs(an) * imu
    nX2 = ar.fmax0(cv * cv * ne + c2["nX2"] * cv * hp + hh)
    s_nX2 = (2 * abs(cv) * s_cv + cv * cv) * ne + 2 * (s_cv * abs(hp) + abs(cv) * s_hp) + s_hh
    nZ2 = s * s * nE2
    s_nZ2 = 2 * s * s_s * nE2 + s * s * s_nE2
    u, u1 = cv - s * az, 1 - s
    s_u, s_u1 = s_cv + s_s * abs(az) + abs(s * az), s_s + 1
    jn2 = ar.fmax0(u * u * ne + c2["jn2"] * u * u1 * hp + u1 * u1 * hh)
    s_jn2 = ((2 * abs(u) * s_u + u * u) * ne + 2 * (s_u * abs(u1 * hp) + abs(u) * s_u1 * abs(hp) + abs(u * u1) * s_hp)
             + 2 * abs(u1) * s_u1 * hh + u1 * u1 * s_hh)
    wz = az * (s - 1)
    s_wz = abs(az) * s_s + abs(wz)
    dZ2 = ar.fmax0(wz * wz * ne + c2["dZ2"] * wz * s * hp + s * s * hh)
    s_dZ2 = ((2 * abs(wz) * s_wz + wz * wz) * ne + 2 * (s_wz * abs(s * hp) + abs(wz) * s_s * abs(hp) + abs(wz * s) * s_hp)
             + 2 * s * s_s * hh + s * s * s_hh)
    # ---- the iteration control (lazy form)
    obj = ar.sqrt(sums["obj2"])
    imp = run & np.asarray(obj < S["opt_obj"], bool)
    rp2 = sums["nJM2"] + jn2
    rp = ar.sqrt(rp2)
    rc2 = rp * rp + sums["dY2"] + dZ2
    rc = ar.sqrt(rc2)
    sc = ys["scale"]
    s_rp2 = sc["nJM2"] + s_jn2
    s_rc2 = s_rp2 + sc["dY2"] + s_dZ2
    tiny = ar.r(1e-300)
    s_rp = s_rp2 / (2 * rp + tiny) + rp
    s_rc = s_rc2 / (2 * rc + tiny) + rc
    nAX, nY, nX, nZ = ar.sqrt(sums["nAX2"]), ar.sqrt(sums["nY2"]), ar.sqrt(nX2), ar.sqrt(nZ2)
    mx1, mx2 = ar.fmax(nAX, nY), ar.fmax(nX, nZ)
    tp = tol_abs * ar.sqrt(ar.r(m + n)) + tol_rel * ar.sqrt(mx1 * mx1 + mx2 * mx2)
    tc = tol_abs * ar.sqrt(ar.r(2 * (m + n))) + tol_rel * ar.sqrt(mx1 * mx1 + mx2 * mx2 + nY * nY + nZ * nZ)
    P, Cc = np.asarray(rp < tp, bool), np.asarray(rc < tc, bool)
    pendn = run & P & ~Cc
    conv = run & ~pendn & Cc
    stop = conv & (not fixed)
    upd = run & ~pendn & ~stop
    bump = upd & np.asarray(rc > S["last_res"] * ar.r(0.9), bool)
    margin["improved"] = np.where(run, rel(obj, S["opt_obj"]), np.nan)
    margin["primal"] = np.where(run, rel(rp, tp), np.nan)
    margin["combined"] = np.where(run, rel(rc, tc), np.nan)
    margin["bump"] = np.where(upd, rel(rc, S["last_res"] * ar.r(0.9)), np.nan)
    margin["shrink"] = np.where(run, rel(nE, imu), np.nan)
    mask.update(imp=imp, pendn=pendn, conv=conv, stop=stop, bump=bump, shrunk0=run & shr0)
    # ---- the control block after the launch
    new = dict(obj2=sums["obj2"], nAX2=sums["nAX2"], nY2=sums["nY2"], nJM2=sums["nJM2"], dY2=sums["dY2"],
               na=az * al, naz=s, nbeta=mu * (1 - s), nep2=nE2)
    for k, v in new.items():
        S[k] = _where(run, v, S[k])
    S["opt_obj"] = _where(imp, obj, S["opt_obj"])
    S["nopt_a"] = _where(imp, cv * al, S["nopt_a"])
    cur = run & ~np.asarray(S["opt_obj"] < ar.inf, bool)
    mask["cur"] = cur
    S["ncur_a"] = _where(cur, cv * al, S["ncur_a"])
    S["pd_dZ2"], S["pd_nZ2"] = _where(pendn, dZ2, S["pd_dZ2"]), _where(pendn, nZ * nZ, S["pd_nZ2"])
    S["pd_rc"] = _where(pendn, rc, S["pd_rc"])
    S["mu"] = _where(bump, mu * rho, mu)
    S["last_res"] = _where(upd, rc, S["last_res"])
    F["iters"] = np.where(run, it, F["iters"])
    F["dpend"] = np.where(pendn, 1, F["dpend"])
    F["status"] = np.where(conv, F["status"] | ST_CONVERGED, F["status"])
    F["done"] = np.where(stop, 1, F["done"])
    done_count += int(stop.sum())
    W = (cv if model != "optW_az" else az)[:, None] * Eo + g
    val.update(Yn=ys["Y"], M=ys["M"], En=En, AEn=AEn, W=W, g=g, T=T, hp=hp, hh=hh, s=s, cv=cv, res_prim=rp, res_comb=rc,
               t_prim=tp, t_comb=tc, jn2=jn2, dZ2=dZ2, nX2=nX2, nZ2=nZ2, **new, nopt_a=cv * al, ncur_a=cv * al,
               pd_dZ2=dZ2, pd_nZ2=nZ * nZ, pd_rc=rc, last_res=rc, opt_obj=obj)
    s_W = s_cv[:, None] * ar.cabs(Eo) + s_g
    scale.update(Yn=sc["Y"], M=sc["M"], En=abs(az)[:, None] * ar.cabs(Eo) + s_g,
                 AEn=abs(az)[:, None] * a_ae + s_T + s_g, W=s_W, g=s_g, obj2=sc["obj2"], nAX2=sc["nAX2"], nY2=sc["nY2"],
                 nJM2=sc["nJM2"], dY2=sc["dY2"], na=abs(az * al), naz=s_s, nbeta=mu * s_s + abs(mu * (1 - s)),
                 nep2=s_nE2, nopt_a=s_cv * abs(al), ncur_a=s_cv * abs(al), pd_dZ2=s_dZ2, pd_nZ2=s_nZ2 + 2 * nZ2,
                 pd_rc=s_rc, last_res=s_rc, res_comb=s_rc, res_prim=s_rp, jn2=s_jn2, dZ2=s_dZ2, nX2=s_nX2, nZ2=s_nZ2,
                 opt_obj=sc["obj2"] / (2 * obj + tiny) + obj)
    return dict(val=val, scale=scale, state=S, flags=F, done_count=done_count, mask=mask, margin=margin)


def mspace_init(Xinit, P0, ar=LD):
    """launch_nms_init: E_prev = X_init (alpha = 1, e = 0, A E_prev = P0), a_z the prox scale at mu = 1, a_n = 0."""
    X = ar.c(Xinit)
    nx0 = _rowsum(ar.abs2(X))
    nz = ar.sqrt(nx0)
    pos = np.asarray(nz > 0, bool)
    naz = _where(pos, ar.fmax0(nz - 1) / _where(pos, nz, nz * 0 + 1), nz * 0)
    return dict(nx0=nx0, nep2=nx0, na=nx0 * 0 + 1, naz=naz, nbeta=nx0 * 0, nopt_a=nx0 * 0, ncur_a=nx0 * 0,
                Eo=ar.c(P0) * 0, AEo=ar.c(P0))


def state_array(b, ar=F64, **kw):
    s = np.zeros((b, len(STATE)), dtype=object if ar.obj else (np.longdouble if ar.kind == "ld" else np.float64))
    if ar.obj:
        s[:] = mp.mpf(0)
    s[:, 0] = 1
    for k, v in kw.items():
        s[:, STATE.index(k)] = v
    return s


def pack_flags(Fl):
    return np.stack([np.asarray(Fl[k]) for k in FLAGS], axis=1).astype(np.int32)


# ---------------------------------------------------------------- (a) the n-space truth
def exact_inverse(K, ar):
    """(I + K)^-1 in ar's arithmetic (mpmath: LU at DPS digits; longdouble: f64 inverse, Newton-refined)."""
    m = K.shape[0]
    if ar.obj:
        Mx = mp.matrix(m, m)
        for i in range(m):
            for j in range(m):
                Mx[i, j] = K[i, j] + (1 if i == j else 0)
        Gi = mp.inverse(Mx)
        return np.array([[Gi[i, j] for j in range(m)] for i in range(m)], dtype=object).reshape(m, m)
    IK = ar.c(K) + np.eye(m)
    G = ar.c(np.linalg.inv(IK.astype(np.complex128)))
    for _ in range(3):
        G = G @ (2 * np.eye(m) - IK @ G)
    return G


@dataclass
class NChain:
    """The n-space truth's chain: ``rec[k]`` is the state after iteration k (k = 0: after init)."""
    A: np.ndarray
    K: np.ndarray
    G: np.ndarray
    Xinit: np.ndarray
    B: np.ndarray
    par: dict
    ar: Arith
    rec: list = field(default_factory=list)

    def mspace(self, k):
        """The kernel's inputs for iteration k + 1, rounded to f64: the state after iteration k in m-space form."""
        r, ar = self.rec[k], self.ar
        b = r["Y"].shape[0]
        st = np.zeros((b, len(STATE)))
        pend = r["pending"]
        get = lambda v: ar.f64(v).astype(np.float64)
        cols = dict(mu=np.where(pend, get(r["mu_used"]), get(r["mu"])),
                    last_res=np.where(pend, get(r["last_res_before"]), get(r["last_res"])),
                    opt_obj=get(r["opt_obj"]), na=get(r["alpha"]), naz=get(r["s"]), nbeta=get(r["an"]),
                    nep2=get(r["nE2"]), nopt_a=get(r["opt_a"]), ncur_a=get(r["cur_a"]),
                    pd_dZ2=np.where(pend, get(r["dZ2"]), 0.0), pd_nZ2=np.where(pend, get(r["nZ2"]), 0.0),
                    pd_rc=np.where(pend, get(r["res_comb"]), 0.0), obj2=get(r["obj2"]), nAX2=get(r["nAX2"]),
                    nY2=get(r["nY2"]), nJM2=get(r["nJM2"]), dY2=get(r["dY2"]), nx0=get(r["nx0"]))
        for kk, v in cols.items():
            st[:, STATE.index(kk)] = v
        fl = np.zeros((b, len(FLAGS)), np.int32)
        fl[:, 0] = r["iters"]
        fl[:, 1] = r["done"] & ~pend          # (a pending stop has not happened yet in the lazy form)
        fl[:, 2] = np.where(pend, r["status_before"], r["status"])
        fl[:, 3] = pend
        c = lambda v: ar.f64(v).astype(np.complex128)
        return dict(G=c(self.G), K=c(self.K), B=get(self.B), Yo=c(r["Y"]), Yn=c(r["Yprev"]), M=c(r["M"]),
                    Eo=c(r["e"]), AEo=c(r["AE"]), optW=c(r["opt_w"]), optY=c(r["opt_Y"]), curW=c(r["cur_w"]),
                    state=st, flags=fl, n=self.A.shape[1], it=k + 1, done_count=int((fl[:, 1] != 0).sum()),
                    **self.par)


def nspace_chain(A, Xinit, Y0, B, iters, *, mu0, rho, tol_rel, tol_abs, fixed_iters, ar=LD):
    """InferADMM (A2nuclear, r = 1) from X = Xinit ([b][n]), Y = Y0 ([b][m]), M = N = 0 on the shared A ([m][n]) for
    `iters` iterations; a realisation that stops keeps its state.  See the module docstring."""
    A_, X, Y, B_ = ar.c(A), ar.c(Xinit), ar.c(Y0), ar.r(B)
    m, n = A_.shape
    b = X.shape[0]
    Ah = ar.conj(A_).T                       # n x m
    K = A_ @ Ah
    G = exact_inverse(K, ar)
    par = dict(rho=rho, tol_rel=tol_rel, tol_abs=tol_abs, fixed_iters=int(bool(fixed_iters)))
    ch = NChain(A=A_, K=K, G=G, Xinit=X, B=B_, par=par, ar=ar)
    rho_, tol_rel_, tol_abs_ = ar.r(rho), ar.r(tol_rel), ar.r(tol_abs)
    zr = _rowsum(ar.abs2(X)) * 0
    nx0 = _rowsum(ar.abs2(X))
    nz = ar.sqrt(nx0)
    pos = np.asarray(nz > 0, bool)
    s0 = _where(pos, ar.fmax0(nz - 1) / _where(pos, nz, zr + 1), zr)
    Z, N, M = s0[:, None] * X, X * 0, Y * 0
    mu, opt_obj, last_res = zr + ar.r(mu0), zr + ar.inf, zr + ar.inf
    done, status, itn = np.zeros(b, bool), np.zeros(b, np.int64), np.zeros(b, np.int64)
    # the kernel's coordinates, booked next to the iterates and never read back by the iteration
    alpha, e, E, s_last, an = zr + 1, Y * 0, X, s0, zr
    opt_a, cur_a, opt_w, cur_w, opt_Y, opt_X = zr, zr, Y * 0, Y * 0, Y * 0, X * 0
    rec0 = dict(Y=Y, Yprev=Y * 0, M=M, e=e, AE=E @ A_.T, alpha=alpha, s=s0, an=an, nE2=nx0, mu=mu, mu_used=mu,
                last_res=last_res, last_res_before=last_res, opt_obj=opt_obj, opt_a=opt_a, cur_a=cur_a, opt_w=opt_w,
                cur_w=cur_w, opt_Y=opt_Y, opt_X=opt_X, X=X, Z=Z, N=N, pending=np.zeros(b, bool), done=done.copy(),
                status=status.copy(), status_before=status.copy(), iters=itn.copy(), nx0=nx0, dZ2=zr, nZ2=zr,
                res_comb=zr, obj2=zr, nAX2=zr, nY2=zr, nJM2=zr, dY2=zr, improved=np.zeros(b, bool),
                bump=np.zeros(b, bool), dual_pass=np.zeros(b, bool), conv=np.zeros(b, bool), Xcur=X)
    ch.rec.append(rec0)
    Xcur = X
    for k in range(1, iters + 1):
        act = ~done
        a1 = act[:, None]
        mu_ = mu[:, None]
        V = Z - N / mu_
        T = (Y - M / mu_) - V @ A_.T
        g = T @ G.T
        Xn = V + g @ Ah.T
        AX = Xn @ A_.T
        C = AX + M / mu_
        d = ar.cabs(C)
        z = d == 0
        C = _where(z, C * 0 + 1, C)
        d = _where(z, d * 0 + 1, d)
        Yn = C * ((B_ / d + mu_) / (1 + mu_))
        En = Xn + N / mu_
        nE2 = _rowsum(ar.abs2(En))
        nE = ar.sqrt(nE2)
        pos = np.asarray(nE > 0, bool)
        s = _where(pos, ar.fmax0(nE - 1 / mu) / _where(pos, nE, zr + 1), zr)
        Zn = s[:, None] * En
        JM, JN = AX - Yn, Xn - Zn
        Mn, Nn = M + mu_ * JM, N + mu_ * JN
        aax = ar.cabs(AX) - B_
        obj2 = _rowsum(aax * aax)
        obj = ar.sqrt(obj2)
        imp = act & np.asarray(obj < opt_obj, bool)
        nJM2, jn2 = _rowsum(ar.abs2(JM)), _rowsum(ar.abs2(JN))
        dY2, dZ2 = _rowsum(ar.abs2(Yn - Y)), _rowsum(ar.abs2(Zn - Z))
        dAtY = _rowsum(ar.abs2((Yn - Y) @ Ah.T))
        nAtY = _rowsum(ar.abs2(Yn @ Ah.T))
        nAX2, nY2, nX2, nZ2 = (_rowsum(ar.abs2(v)) for v in (AX, Yn, Xn, Zn))
        rp = ar.sqrt(nJM2 + jn2)
        rd = mu * ar.sqrt(dAtY + dZ2)
        rc = ar.sqrt(rp * rp + dY2 + dZ2)
        mx1, mx2 = ar.fmax(nAX2, nY2), ar.fmax(nX2, nZ2)
        tp = tol_abs_ * ar.sqrt(ar.r(m + n)) + tol_rel_ * ar.sqrt(mx1 + mx2)
        td = tol_abs_ * ar.sqrt(ar.r(2 * n)) + tol_rel_ * ar.sqrt(nAtY + nZ2)
        tc = tol_abs_ * ar.sqrt(ar.r(2 * (m + n))) + tol_rel_ * ar.sqrt(mx1 + mx2 + nY2 + nZ2)
        P, D, Cc = (np.asarray(x, bool) for x in (rp < tp, rd < td, rc < tc))
        pending = act & P & ~Cc
        conv = act & ((P & D) | Cc)
        stop = conv & (not fixed_iters)
        upd = act & ~stop
        bump = upd & np.asarray(rc > last_res * ar.r(0.9), bool)
        # the kernel's coordinates of this iteration
        az_prev = s_last
        cvk = az_prev - an / mu
        e_new = az_prev[:, None] * e + g
        w_new = cvk[:, None] * e + g
        status_before = status.copy()
        last_before = last_res
        mu_used = mu
        # commit (stopped realisations keep their state; the stopping iteration's iterate is committed)
        Yprev = _where(a1, Y, ch.rec[-1]["Yprev"])
        Y, M, Z, N = _where(a1, Yn, Y), _where(a1, Mn, M), _where(a1, Zn, Z), _where(a1, Nn, N)
        Xcur = _where(a1, Xn, Xcur)
        E, e = _where(a1, En, E), _where(a1, e_new, e)
        alpha = _where(act, az_prev * alpha, alpha)
        cva = cvk * ch.rec[-1]["alpha"]
        s_last, an = _where(act, s, s_last), _where(act, mu * (1 - s), an)
        opt_obj = _where(imp, obj, opt_obj)
        i1 = imp[:, None]
        opt_X, opt_Y, opt_w = _where(i1, Xn, opt_X), _where(i1, Yn, opt_Y), _where(i1, w_new, opt_w)
        opt_a = _where(imp, cva, opt_a)
        cur = act & ~np.asarray(opt_obj < ar.inf, bool)
        cur_w, cur_a = _where(cur[:, None], w_new, cur_w), _where(cur, cva, cur_a)
        status = np.where(conv, status | ST_CONVERGED, status)
        done = done | stop
        itn = np.where(act, k, itn)
        mu = _where(bump, mu * rho_, mu)
        last_res = _where(upd, rc, last_res)
        keep = lambda new, name: _where(act, new, ch.rec[-1][name])
        ch.rec.append(dict(
            Y=Y, Yprev=Yprev, M=M, e=e, AE=E @ A_.T, alpha=alpha, s=s_last, an=an, nE2=keep(nE2, "nE2"), mu=mu,
            mu_used=keep(mu_used, "mu_used"), last_res=last_res, last_res_before=keep(last_before, "last_res_before"),
            opt_obj=opt_obj, opt_a=opt_a, cur_a=cur_a, opt_w=opt_w, cur_w=cur_w, opt_Y=opt_Y, opt_X=opt_X, X=Xcur,
            Z=Z, N=N, pending=pending, done=done.copy(), status=status.copy(), status_before=status_before,
            iters=itn.copy(), nx0=nx0, dZ2=keep(dZ2, "dZ2"), nZ2=keep(nZ2, "nZ2"), res_comb=keep(rc, "res_comb"),
            obj2=keep(obj2, "obj2"), nAX2=keep(nAX2, "nAX2"), nY2=keep(nY2, "nY2"), nJM2=keep(nJM2, "nJM2"),
            dY2=keep(dY2, "dY2"), improved=imp, bump=bump, dual_pass=pending & D, conv=conv, Xcur=Xcur,
            jn2=jn2, nX2=nX2, res_prim=rp, res_dual=rd, dAtY=dAtY, nAtY=nAtY, t_prim=tp, t_dual=td, t_comb=tc,
            g=g, T=T, act=act))
    return ch


# ---------------------------------------------------------------- problems and the suite's inputs
def problem(seed, m, n, b):
    """A genuine small phase-retrieval problem: complex A with ||A||_F = sqrt(m) and a non-trivial imaginary part
    (K = A A^H is not symmetric), B = |A x| with noise, normalised to ||B|| = 1, and the solver's starting point
    (X_init scaled to ||A X|| = ||B||, Y0 = A X_init with the rows' magnitudes set to B).  Every realisation differs."""
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))) / np.sqrt(2 * n)
    x = rng.standard_normal((b, n)) + 1j * rng.standard_normal((b, n))
    x *= (1 + np.arange(b))[:, None] ** 0.25
    Bm = np.abs(x @ A.T) * (1 + 0.03 * rng.standard_normal((b, m)))
    Bm = np.abs(Bm) / np.sqrt(np.sum(Bm * Bm, axis=1))[:, None]
    X0 = x + 0.5 * (rng.standard_normal((b, n)) + 1j * rng.standard_normal((b, n)))
    AX = X0 @ A.T
    X0 = X0 * (np.sqrt(np.sum(Bm * Bm, axis=1)) / np.sqrt(np.sum(np.abs(AX) ** 2, axis=1)))[:, None]
    AX = X0 @ A.T
    Y0 = AX * (Bm / np.abs(AX))
    return A, Bm, X0, Y0


DEFAULT = dict(mu0=4.0, rho=1.05, tol_rel=1e-4, tol_abs=1e-8, fixed_iters=False)


@functools.lru_cache(maxsize=None)
def chain(seed, m, n, b, iters, mu0=4.0, rho=1.05, tol_rel=1e-4, fixed_iters=False, x_scale=1.0):
    A, B, X0, Y0 = problem(seed, m, n, b)
    return nspace_chain(A, X0 * x_scale, Y0, B, iters, mu0=mu0, rho=rho, tol_rel=tol_rel, tol_abs=1e-8,
                        fixed_iters=fixed_iters, ar=LD)


# name -> (seed, m, n, batch, k: the state is the chain's after iteration k (None: its first pending one), the
# chain's options, the launch's own control parameters where they differ from the chain's)
# (On the reference's own chains a pending test always fails its dual part -- the combined test passes first -- so the
# two inputs that exercise a passing one finish a pending state of the chain under a larger tol_rel of the launch.)
CASES = {
    "m1-n4-b1-k0": (1, 1, 4, 1, 0, {}, {}),
    "m16-n16-b15-k1": (2, 16, 16, 15, 1, {}, {}),
    "m31-n16-b16-k5": (3, 31, 16, 16, 5, {}, {}),
    "m33-n16-b17-k30": (4, 33, 16, 17, 30, dict(fixed_iters=True), {}),
    "m40-n16-b33-k1-done": (5, 40, 16, 33, 1, {}, {}),
    "m40-n4-b17-k5-alldone": (6, 40, 4, 17, 5, {}, {}),
    "m121-n16-b17-k0": (14, 121, 16, 17, 0, {}, {}),
    "m121-n64-b16-k30": (7, 121, 64, 16, 30, dict(fixed_iters=True), {}),
    "m225-n64-b15-k5": (8, 225, 64, 15, 5, {}, {}),
    "m256-n64-b16-k1": (9, 256, 64, 16, 1, {}, {}),
    "m256-n64-b17-k5-mu1e-3": (10, 256, 64, 17, 5, dict(mu0=1e-3), {}),
    "m40-n16-b16-fixpoint": (11, 40, 16, 16, 40, dict(rho=2.0, fixed_iters=True), {}),
    "m40-n16-b16-fixpoint-stop": (11, 40, 16, 16, 40, dict(rho=2.0, fixed_iters=True), dict(fixed_iters=0)),
    "m256-n64-b16-fixpoint": (12, 256, 64, 16, 40, dict(rho=2.0, fixed_iters=True), {}),
    "m33-n16-b17-pending": (13, 33, 16, 17, None, dict(tol_rel=3e-2), {}),
    "m33-n16-b17-pending-bump": (13, 33, 16, 17, 57, {}, {}),
    "m33-n16-b17-pending-pass": (13, 33, 16, 17, 6, dict(tol_rel=3e-2), dict(tol_rel=0.3)),
    "m33-n16-b17-pending-pass-fixed": (13, 33, 16, 17, 6, dict(tol_rel=3e-2, fixed_iters=True),
                                       dict(tol_rel=0.3)),
    "m40-n16-b17-k0-nanB": (15, 40, 16, 17, 0, {}, {}),
    # past init (e != 0, a_n != 0, c_v != a_z) with opt_obj = +inf: every realisation records its iterate, and the one
    # with a NaN in B keeps it as the current iterate
    "m121-n64-b16-k30-imp": (7, 121, 64, 16, 30, dict(fixed_iters=True), dict(opt_inf=True)),
    "m33-n16-b17-k5-imp-nanB": (16, 33, 16, 17, 5, {}, dict(opt_inf=True)),
    # the launch's tol_rel set between the values at which the combined test ties with ||X||^2 as it is and with the
    # factor 2 of its middle term missing (realisation NX2_ROW): the form decides converged / not there
    "m31-n16-b16-k5-nX2": (3, 31, 16, 16, 5, dict(mu0=1e-3), dict(tol_between="hp1_nX2")),
}
DONE_ROWS = {"m40-n16-b33-k1-done": (5, 20, 21, 22), "m40-n4-b17-k5-alldone": tuple(range(16))}
NAN_B = {"m40-n16-b17-k0-nanB": (3, 7), "m33-n16-b17-k5-imp-nanB": (9, 2)}      # (realisation, row) of a NaN in B
NX2_ROW = 0


def _first_pending(ch):
    for k, r in enumerate(ch.rec):
        if r["pending"].any():
            return k
    raise AssertionError("the chain never leaves a convergence test pending")


@functools.lru_cache(maxsize=None)
def case(name):
    """The kernel's inputs of a named case (a dict for ``mspace_step`` / ``ace_amd.nms.nms_host('step', ...)``)."""
    seed, m, n, b, k, opt, over = CASES[name]
    iters = 60 if k is None else k
    ch = chain(seed, m, n, b, iters, **opt)
    if k is None:
        k = _first_pending(ch)
    inp = ch.mspace(k)
    over = dict(over)
    if over.pop("opt_inf", False):
        inp["state"][:, STATE.index("opt_obj")] = np.inf
    between = over.pop("tol_between", None)
    inp.update(over)
    if between:
        inp["tol_rel"] = tie_between(inp, between, NX2_ROW)
    for j in DONE_ROWS.get(name, ()):
        inp["flags"][j, FLAGS.index("done")] = 1
    if name in NAN_B:
        inp["B"][NAN_B[name]] = np.nan
    inp["done_count"] = int((inp["flags"][:, FLAGS.index("done")] != 0).sum())
    inp["name"] = name
    return inp


def _comb_tie(o, inp, j):
    """The tol_rel at which realisation j's combined test ties: res_comb = tol_abs c + tol_rel (threshold norm)."""
    v = o["val"]
    m = np.asarray(inp["Yo"]).shape[1]
    norm = (v["t_comb"][j] - LD.r(inp["tol_abs"]) * np.sqrt(LD.r(2 * (m + inp["n"])))) / LD.r(inp["tol_rel"])
    return float((v["res_comb"][j] - LD.r(inp["tol_abs"]) * np.sqrt(LD.r(2 * (m + inp["n"])))) / norm)


def tie_between(inp, model, j):
    """A tol_rel between the combined test's ties of realisation j under the right step and under `model`."""
    a, b = _comb_tie(mspace_step(inp), inp, j), _comb_tie(mspace_step(inp, model=model), inp, j)
    assert abs(a - b) > 1e-2 * max(a, b), (a, b)
    return float(np.sqrt(a * b))


def rows(inp, idx):
    """The same launch on a subset of the realisations."""
    idx = np.asarray(idx)
    out = dict(inp)
    for k in ("B", "Yo", "Yn", "M", "Eo", "AEo", "optW", "optY", "curW", "state", "flags"):
        if out.get(k) is not None:
            out[k] = np.asarray(out[k])[idx]
    return out


# ---------------------------------------------------------------- (b) chained: init, steps, fin, out
def mspace_chain(G, K, A, B, Xinit, Y0, iters, *, mu0, rho, tol_rel, tol_abs, fixed_iters, ar=LD, model=None):
    """``mspace_step`` chained from ``mspace_init`` the way the solve chains the kernel's launches (ping-pong buffers,
    fin and out at the end); P0 = A X_init is formed in ar's arithmetic.  Returns the per-step results (each with
    ``vec``: the buffers after the step, as the next step reads them) and the final dict (X, mu, iters, status, done)."""
    A_, X0 = ar.c(A), ar.c(Xinit)
    ini = mspace_init(X0, X0 @ A_.T, ar)
    b, m = np.asarray(Y0).shape
    n = A_.shape[1]
    st = state_array(b, ar)
    for k_, v in dict(mu=ar.r(mu0), last_res=ar.inf, opt_obj=ar.inf, na=ini["na"], naz=ini["naz"], nbeta=ini["nbeta"],
                      nep2=ini["nep2"], nx0=ini["nx0"]).items():
        st[:, STATE.index(k_)] = v
    fl = np.zeros((b, len(FLAGS)), np.int32)
    zero = ar.c(Y0) * 0
    buf = dict(Yo=ar.c(Y0), Yn=zero, M=zero, Eo=ini["Eo"], En=zero, AEo=ini["AEo"], AEn=zero, optW=zero, optY=zero,
               curW=zero)
    par = dict(G=G, K=K, B=B, n=n, rho=rho, tol_rel=tol_rel, tol_abs=tol_abs, fixed_iters=int(bool(fixed_iters)))
    dc, steps = 0, []
    for it in range(1, iters + 1):
        o = mspace_step(dict(par, state=st, flags=fl, it=it, done_count=dc, **buf), ar, model=model)
        run, v = o["mask"]["run"][:, None], o["val"]
        imp, cur = o["mask"]["imp"][:, None], o["mask"]["cur"][:, None]
        Yn, En, AEn = _where(run, v["Yn"], buf["Yn"]), _where(run, v["En"], buf["En"]), _where(run, v["AEn"], buf["AEn"])
        buf = dict(Yo=Yn, Yn=buf["Yo"], M=_where(run, v["M"], buf["M"]), Eo=En, En=buf["Eo"], AEo=AEn, AEn=buf["AEo"],
                   optW=_where(imp, v["W"], buf["optW"]), optY=_where(imp, v["Yn"], buf["optY"]),
                   curW=_where(cur, v["W"], buf["curW"]))
        st, fl, dc = np.stack([o["state"][k_] for k_ in STATE], axis=1), pack_flags(o["flags"]), o["done_count"]
        o["vec"] = dict(buf)
        steps.append(o)
    o = mspace_step(dict(par, state=st, flags=fl, it=iters, done_count=dc, **buf), ar, fin=True)
    S, Fl = o["state"], o["flags"]
    have = np.asarray(S["opt_obj"] < ar.inf, bool)
    co = _where(have, S["nopt_a"], S["ncur_a"])
    Wsel = _where(have[:, None], buf["optW"], buf["curW"])
    X = co[:, None] * X0 + Wsel @ ar.conj(A_)
    return steps, dict(X=X, V=co[:, None] * X0, Wsel=Wsel, mu=S["mu"], iters=Fl["iters"], status=Fl["status"],
                       done=Fl["done"], done_count=o["done_count"], state=S, flags=Fl, fin=o, have=have)


# ---------------------------------------------------------------- what a launch leaves, and how it is compared
SI = {k: i for i, k in enumerate(STATE)}
FI = {k: i for i, k in enumerate(FLAGS)}


def model_result(inp, model=None, ar=F64, fin=False):
    """The buffers and control blocks a launch of ``mspace_step(inp, ar, model)`` would leave on the device (the layout
    ``compare_step`` reads: vec, state, flags, done_count), every unwritten row as the input has it."""
    with np.errstate(all="ignore"):
        o = mspace_step(inp, ar, model=model, fin=fin)
    b, m = np.asarray(inp["Yo"]).shape
    nan = np.full((b, m), np.nan + 0j)
    vec = {k: np.array(inp[k], np.complex128) for k in ("Yo", "Yn", "M", "Eo", "AEo", "optW", "optY", "curW")}
    vec.update(En=nan.copy(), AEn=nan.copy(), B=np.array(inp["B"], np.float64))
    if not fin:
        run, imp, cur = (o["mask"][k][:, None] for k in ("run", "imp", "cur"))
        val = {k: ar.f64(o["val"][k]) for k in ("Yn", "M", "En", "AEn", "W")}
        for k in ("Yn", "M", "En", "AEn"):
            vec[k] = np.where(run, val[k], vec[k])
        vec["optW"], vec["optY"] = np.where(imp, val["W"], vec["optW"]), np.where(imp, vec["Yn"], vec["optY"])
        vec["curW"] = np.where(cur, val["W"], vec["curW"])
    state = np.stack([ar.f64(o["state"][k]).astype(np.float64) for k in STATE], axis=1)
    return types.SimpleNamespace(vec=vec, state=state, flags=pack_flags(o["flags"]), done_count=o["done_count"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.all(_bits(a) == _bits(b)))


def compare_step(got, inp, fin=False):
    """Every comparison of one launch's results (``got``: vec, state, flags, done_count) with (b) on ``inp``.
    Returns (ratios, broken, ref): ratios is a list of (output, worst err / tol over the rows compared), broken the
    names of the exact comparisons that do not hold (decisions, mu, rows that must keep their contents).  The GPU
    suite asserts every ratio <= 1 and nothing broken; the self-test measures the wrong-step models through the same
    function, so a model counts as caught only by what the device run compares."""
    ref = mspace_step(inp, LD, fin=fin)
    msk, val, sc = ref["mask"], ref["val"], ref["scale"]
    run, live = msk["run"], msk["live"]
    b, m = np.asarray(inp["Yo"]).shape
    st_in, fl_in = np.asarray(inp["state"]), np.asarray(inp["flags"])
    S = lambda k: got.state[:, SI[k]]
    ratios, broken = [], []

    def within(x, r, scale, rws, out):
        x, r = np.asarray(x)[rws].astype(np.clongdouble), np.asarray(r)[rws].astype(np.clongdouble)
        if not x.size:
            return
        tol = tolerance(np.asarray(scale)[rws])
        err = np.abs(x - r)
        with np.errstate(all="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
        ratio = np.where(np.isfinite(x.real) & np.isfinite(x.imag), ratio, np.inf)
        ratios.append((out, float(ratio.max())))

    def exact(cond, name):
        if not cond:
            broken.append(name)

    nanrow = run & np.isnan(LD.f64(val["obj2"]).astype(np.float64)) if not fin else np.zeros(b, bool)
    ok = run & ~nanrow
    # ---- the read-only inputs and the rows the launch does not run
    for k in ("B", "Yo", "Eo", "AEo"):
        exact(same_bits(got.vec[k], inp[k]), "input " + k)
    idle = ~run
    exact(same_bits(got.vec["Yn"][idle], np.asarray(inp["Yn"])[idle]), "Yn of idle rows")
    exact(same_bits(got.vec["M"][idle], np.asarray(inp["M"])[idle]), "M of idle rows")
    exact(same_bits(got.state[~live], st_in[~live]) and np.array_equal(got.flags[~live], fl_in[~live]),
          "control block of done rows")
    # ---- 3: the pending tests on entry
    pin = msk["pend_in"]
    within(S("dAtY"), ref["state"]["dAtY"], sc.get("dAtY", 0), pin, "dAtY") if pin.any() else None
    within(S("nAtY"), ref["state"]["nAtY"], sc.get("nAtY", 0), pin, "nAtY") if pin.any() else None
    # ---- decisions, exactly
    for k in FLAGS:
        exact(np.array_equal(got.flags[:, FI[k]], ref["flags"][k]), "flag " + k)
    exact(got.done_count == ref["done_count"], "done_count")
    rho = np.float64(inp["rho"])
    mu0 = st_in[:, SI["mu"]]
    mu1 = np.where(msk["bump_in"], mu0 * rho, mu0)
    mu2 = np.where(msk["bump"], mu1 * rho, mu1)
    exact(same_bits(S("mu"), mu2), "mu")
    cont_in = pin & ~msk["stop_in"]
    upd = run & ~msk["pendn"] & ~msk["stop"]
    lr1 = np.where(cont_in, st_in[:, SI["pd_rc"]], st_in[:, SI["last_res"]])
    keep = (~(upd & ~nanrow) if not fin else np.ones(b, bool)) & ~nanrow
    exact(same_bits(S("last_res")[keep], lr1[keep]), "last_res of rows that keep it")
    if fin:
        for k in ("Yn", "M", "optW", "optY", "curW"):
            exact(same_bits(got.vec[k], inp[k]), "fin wrote " + k)
        cols = [SI[k] for k in STATE if k not in ("mu", "last_res", "dAtY", "nAtY")]
        exact(same_bits(got.state[:, cols], st_in[:, cols]), "fin changed the iteration's state")
        return ratios, broken, ref
    # ---- 1: the step against (b)
    for k in ("Yn", "M", "En", "AEn"):
        within(got.vec[k], val[k], sc[k], ok, k)
    for k in ("obj2", "nAX2", "nY2", "nJM2", "dY2", "naz", "nbeta", "na", "nep2"):
        within(S(k), val[k], sc[k], ok, k)
    within(S("last_res"), val["res_comb"], sc["res_comb"], upd & ok, "last_res")
    pn = msk["pendn"]
    for k in ("pd_dZ2", "pd_nZ2", "pd_rc"):
        within(S(k), val[k], sc[k], pn, k)
        exact(same_bits(S(k)[~pn], st_in[~pn, SI[k]]), k + " of rows not pending")
    z0 = msk["shrunk0"] & ok                      # 4: ||E_new|| < 1/mu gives s = 0 exactly
    exact(bool(np.all(S("naz")[z0] == 0.0)) and same_bits(S("nbeta")[z0], mu1[z0]), "shrink to zero")
    # ---- 2: the recorded iterates
    imp, cur = msk["imp"], msk["cur"]
    within(got.vec["optW"], val["W"], sc["W"], imp, "optW")
    within(S("nopt_a"), val["nopt_a"], sc["nopt_a"], imp, "nopt_a")
    within(S("opt_obj"), val["opt_obj"], sc["opt_obj"], imp, "opt_obj")
    exact(same_bits(got.vec["optY"][imp], got.vec["Yn"][imp]), "opt_Y = Y_new")
    exact(same_bits(got.vec["optW"][~imp], np.asarray(inp["optW"])[~imp]), "optW without an improvement")
    exact(same_bits(got.vec["optY"][~imp], np.asarray(inp["optY"])[~imp]), "optY without an improvement")
    exact(same_bits(S("opt_obj")[~imp], st_in[~imp, SI["opt_obj"]]), "opt_obj without an improvement")
    exact(same_bits(S("nopt_a")[~imp], st_in[~imp, SI["nopt_a"]]), "nopt_a without an improvement")
    within(got.vec["curW"], val["W"], sc["W"], cur, "curW")
    within(S("ncur_a"), val["ncur_a"], sc["ncur_a"], cur, "ncur_a")
    exact(same_bits(got.vec["curW"][~cur], np.asarray(inp["curW"])[~cur]), "curW with a finite objective")
    exact(same_bits(S("ncur_a")[~cur], st_in[~cur, SI["ncur_a"]]), "ncur_a with a finite objective")
    # a NaN objective: nothing finite is claimed for the Y side; the X side is compared
    if nanrow.any():
        exact(bool(np.all(np.isnan(S("obj2")[nanrow])) and np.all(cur[nanrow]) and not imp[nanrow].any()), "NaN objective")
        for k in ("En", "AEn"):
            within(got.vec[k], val[k], sc[k], nanrow, k)
        for k in ("naz", "nep2", "na", "nbeta"):
            within(S(k), val[k], sc[k], nanrow, k)
    return ratios, broken, ref


# the inputs whose step records its iterate past init; the f64 transcription's own deviation of V + A^H Wsel from the
# n-space truth's X there (tests/test_nms_ref.py::test_recorded_iterate_deviation prints it), the kernel gets 8 x
RECORDED = ("m121-n64-b16-k30-imp", "m33-n16-b17-k5-imp-nanB")
REC_DEV = 4.5e-16


def recorded_truth(name):
    """A, X_init and the n-space truth's X of the iteration the named input's step runs."""
    seed, m, n, b, k, opt, _ = CASES[name]
    ch = chain(seed, m, n, b, k + 1, **opt)
    A, _, X0, _ = problem(seed, m, n, b)
    return A, X0, ch.rec[k + 1]["Xcur"]


def recorded_deviation(V, Wsel, A, truth):
    X = np.asarray(V).astype(np.clongdouble) + np.asarray(Wsel).astype(np.clongdouble) @ np.conj(LD.c(A))
    nrm = lambda x: np.sqrt(np.sum(np.abs(x) ** 2, axis=1))
    return float(np.max(nrm(X - truth) / nrm(truth)))


# the chains of assertion 6: name -> (seed, m, n, batch); the solver's default control parameters
CHAINS = {"m40-n16-b17": (41, 40, 16, 17), "m256-n64-b16": (42, 256, 64, 16)}
CHAIN_PAR = dict(mu0=4.0, rho=1.05, tol_rel=1e-4, tol_abs=1e-8, fixed_iters=False)
CHAIN_STEPS = 5


def chain_deviation(steps, fin, ch):
    """Relative deviations of a chained run (the spec's, or the kernel's in the same layout) from the n-space truth."""
    nrm = lambda x: np.sqrt(np.sum(np.abs(np.asarray(x).astype(np.clongdouble)) ** 2, axis=-1))
    dy = dx = ds = 0.0
    for k, o in enumerate(steps, 1):
        r = ch.rec[k]
        dy = max(dy, float(np.max(nrm(np.asarray(o["val"]["Yn"]).astype(np.clongdouble) - r["Y"]) / nrm(r["Y"]))))
        for a_, b_ in (("nep2", "nE2"), ("naz", "s"), ("res_comb", "res_comb")):
            ds = max(ds, float(np.max(np.abs(np.asarray(o["val"][a_]).astype(np.longdouble) - r[b_]) / np.abs(r[b_]))))
    last = ch.rec[len(steps)]
    dx = float(np.max(nrm(np.asarray(fin["X"]).astype(np.clongdouble) - last["opt_X"]) / nrm(last["opt_X"])))
    return dict(y=dy, x=dx, scal=ds)


def tolerance(scale):
    return TOL_MULT * U * np.asarray(scale, np.longdouble)
