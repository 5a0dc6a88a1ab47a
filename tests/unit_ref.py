"""References, inputs and derived tolerances for the unit path's fused iteration kernels (csrc/ace_i8gemm.hip: gyk_kernel,
gyf_kernel, msr_kernel, the fused epilogue of i8ah_kernel, msr_ready_kernel, launch_i8_msp_optx; tests/test_gpu_unit.py,
self-tested on the CPU by tests/test_unit_ref.py).  Nothing here calls project code.

(b) the kernels' specification
------------------------------
``step`` evaluates one launch (gyk, gyf or the stand-alone fused apply_AH) on exactly the f64 inputs the launch got,
with the c, G and K the setup made, in longdouble (or plain f64: the same function): the pending convergence tests
(dual_finish) and the T that follows the new mu, the deferred opt_Y / opt_S saves, T = (Y - M/mu) - A V (AX taken
for A V where the previous X is V), g = G T, ArgMinY with its zero guard and the M update (``nms_ref.ystep``), the five
sums, the two m-space sums Re (A Z)^H g and g^H K g = Re g^H (T - g), S' = S + g, the entry bound with `room`,
fused_control -> iter_control_in, the opt_Y / opt_S / optsrc / optysrc bookkeeping, X = Z + c A^H g with fs0 / fs3,
and K Y' with dAtY / nAtY.  ``run`` iterates it with msr_kernel's stop rules, write-back and counters; ``ready`` and
``optx`` are the two helpers.  Every output comes with an absolute error scale S = kappa |value| (first-order
propagation, as nms_ref: a sum of |terms| for a sum, so kappa grows where a value cancels: the fs0 update, g^H K g,
res_comb, dAtY as a difference) and, where an int8 digit-plane product feeds it (apply_A into T, A^H g, K Y), an
additive term from ``linop_ref.i8_tol`` as it stands, propagated the same way.

Tolerance: TOL_MULT u S + (propagated int8 term), u = 2^-53.  TOL_MULT is not chosen by looking at the kernels:
tests/test_unit_ref.py measures the largest err / (u S) of the f64 transcription (``step(..., ar=F64)``) against the
longdouble one over the suite's inputs, floors it at 1, asserts it stays below ORACLE_RATIO, and the kernels get
8 x ORACLE_RATIO (the device's other summation order: 16-lane butterflies, eight waves in fixed order, 3M products).

(a) the n-space truth
---------------------
``nspace_step`` is one InferADMM A2only iteration (inferLowRankV4_multi.m:318-342, ArgMinY through
oracle/ace_oracle.py) in longdouble with Z explicit: for a realisation in m-space form Z = Z0 + A^H S.  X = V + A^H g*
with g* the longdouble solution of (I + K) g = T (``linop_ref.g_reference``), so it shares neither G nor the m-space
identities with the kernels.  ``compare_truth`` bounds the kernels' distance from it by (b)'s tolerance with
||G - (I + K)^-1||_inf ||T||_inf and the measured inconsistency of the inputs (AX against A V, fs0 against ||Z||^2)
added to the propagated term.
"""
import functools
import pathlib
import sys

import numpy as np

import linop_ref as L
from nms_ref import LD, F64, ystep, _rowsum

U = 2.0 ** -53
# largest err / (u S) of the f64 transcription over the suite's inputs, floored at 1 and rounded up (measured 6.087 at
# gykT-m121-n256-b35, g = G T of a given T; 2.1 for nAtY, below 1 elsewhere: tests/test_unit_ref.py::test_oracle_ratio
# prints them), and the kernels' multiplier
ORACLE_RATIO = 6.1
TOL_MULT = 8.0 * ORACLE_RATIO

STATE = ("mu", "last_res", "opt_obj", "nB", "vbound", "obj2", "nAX2", "nY2", "nJM2", "dY2", "dAtY", "nAtY", "kf0",
         "kf1", "kf2", "kf3", "kfcum", "pd_dZ2", "pd_nZ2", "pd_rc", "fs0", "fs3")
FLAGS = ("iters", "done", "status", "nzero", "avok", "optsrc", "optysrc", "kfok", "dpend", "fzit", "zit", "mzit", "msp",
         "z0id", "msp_pad", "mres")
VEC_M = ("T", "g", "Y0", "Y1", "KY0", "KY1", "M", "AX", "optY", "S0", "S1", "optS")
VEC_N = ("Zb1", "Zb2", "Nb1", "Nb2", "X", "Xcur", "optX")
ST_CONVERGED = 1
MODELS = ("stale_mu", "S_not_reset", "optY_from_Yo", "pad_in_sums", "fs0_no_2", "fs3_from_gg", "kfcum_no_room",
          "wb_parity", "resume_plus1", "no_zero_guard")
PAR = dict(tol_rel=1e-4, tol_abs=1e-8, rho=1.05, fixed_iters=0, maxiter=1 << 30, lazy=1, use_la=1, use_ax=1, yn_copy=0,
           msp=0, ctl=1, np=0, fl=(), room=32.0, msp_fail_it=-1, done_count=0, mspcount=0, waves=8, it_end=0)


def state_array(b, **kw):
    s = np.zeros((b, len(STATE)))
    s[:, 0] = 1.0
    for k, v in kw.items():
        s[:, STATE.index(k)] = v
    return s


def flags_array(b, **kw):
    f = np.zeros((b, len(FLAGS)), np.int32)
    for k, v in kw.items():
        f[:, FLAGS.index(k)] = v
    return f


def tolerance(scale, extra=0.0):
    return TOL_MULT * U * np.asarray(scale, np.longdouble) + np.asarray(extra, np.longdouble)


def _w(mask, a, b):
    mask = np.asarray(mask, bool)
    if np.ndim(a) == 2 or np.ndim(b) == 2:
        mask = mask[:, None] if mask.ndim == 1 else mask
    return np.where(mask, a, b)


def _cabs_tol(t):
    """Per-real-component tolerances [nv][2k] -> one per complex entry [nv][k]."""
    t = np.asarray(t, np.float64)
    return np.hypot(t[:, 0::2], t[:, 1::2])


def operators(A):
    """K = A A^H and G = (I + K)^-1 in f64 and c = (c, c^2) as a CPU stand-in for what the setup returns (the GPU tests
    put the setup's own K, G, c in their place: ``with_ops``)."""
    c, P, Q = L.phase_parts(A)
    kr, ki = L.kint(A)
    K = (c * c) * (kr + 1j * ki)
    G = np.linalg.inv(np.eye(A.shape[0]) + K)
    return dict(K=K, G=0.5 * (G + G.conj().T), c=np.array([c, c * c]))


def with_ops(inp, K, G, c):
    out = dict(inp)
    out.update(K=np.asarray(K), G=np.asarray(G), c=np.asarray(c, np.float64))
    return out


class _Ops:
    """Integer parts of the codebook and the exact operators built from the c the kernels use."""

    def __init__(self, inp, ar):
        A = np.asarray(inp["A"], np.complex128)
        _, P, Q = L.phase_parts(A)
        self.m, self.n = A.shape
        self.c, self.c2 = float(inp["c"][0]), float(inp["c"][1])
        self.PQ = P + 1j * Q
        self.A = ar.r(self.c) * ar.c(self.PQ)
        kr, ki = L.kint(A)
        self.Kint = kr + 1j * ki
        self.K = ar.r(self.c2) * ar.c(self.Kint)
        self.G = ar.c(inp["G"])
        self.EA = L.real_expand(self.PQ)
        self.EAH = L.real_expand(self.PQ.conj().T)
        self.EK = L.real_expand(self.Kint)
        self.absA = self.c * (np.abs(P) + np.abs(Q)).astype(np.float64)
        self.absK = self.c2 * (np.abs(kr) + np.abs(ki)).astype(np.float64)
        self.ar = ar

    def i8(self, E, scale, V, prod, bound=None):
        """linop_ref's int8 tolerance of scale E V per complex output, the exponent from `bound` (default max |V|)."""
        V64 = F64.c(self.ar.f64(V))
        bnd = L.maxabs_rows(V64) if bound is None else np.asarray(bound, np.float64)
        bnd = np.where(np.isfinite(bnd), bnd, 0.0)
        hi = np.ascontiguousarray(F64.c(self.ar.f64(prod))).view(np.float64)
        return _cabs_tol(L.i8_tol(E, scale, L.kernel_exp(bnd), hi))


def _load(inp, ar):
    st = np.asarray(inp["state"], np.float64)
    S = {k: ar.r(st[:, i]) for i, k in enumerate(STATE)}
    fl = np.asarray(inp["flags"]).astype(np.int64)
    F = {k: fl[:, i].copy() for i, k in enumerate(FLAGS)}
    return S, F


def _rel(ar, a_, b_):
    a64, b64 = ar.f64(a_).astype(np.float64), ar.f64(b_).astype(np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(a64 - b64) / np.maximum(np.abs(a64), np.abs(b64))
    return np.where(np.isinf(a64) | np.isinf(b64), np.inf, d)


def _profile(inp, b):
    """Per realisation: (np, fl[4]) of z_profile."""
    r1 = np.zeros(b, bool) if inp.get("rank_one") is None else np.asarray(inp["rank_one"]).astype(bool)
    fl = np.zeros((b, 4))
    fl[:, :len(inp["fl"])] = np.asarray(inp["fl"], np.float64)[None, :]
    fl[r1] = np.array([0.95, 0.0, 0.0, 0.0])
    return np.where(r1, 1, int(inp["np"])), fl


def _bound(ar, S, s0, cum, npv, flv, rows, margin, key):
    """pass = s0 > 0 and for p < np: lb = kf[p] (1 - 1e-12) - cum > 0 and lb^2 > fl[p] s0 (1 + 1e-9)."""
    ok = np.asarray(s0 > 0, bool)
    mg = np.full(len(ok), np.inf)
    for p in range(4):
        use = rows & (p < npv)
        lb = S[f"kf{p}"] * ar.r(1.0 - 1e-12) - cum
        rhs = ar.r(flv[:, p]) * s0 * ar.r(1.0 + 1e-9)
        okp = np.asarray(lb > 0, bool) & np.asarray(lb * lb > rhs, bool)
        ok = ok & np.where(use, okp, True)
        with np.errstate(all="ignore"):
            mp_ = np.minimum(_rel(ar, lb * lb, rhs), np.abs(ar.f64(lb).astype(np.float64)) /
                             np.maximum(np.abs(ar.f64(S[f"kf{p}"]).astype(np.float64)), 1e-300))
        mg = np.where(use, np.minimum(mg, np.where(np.asarray(lb > 0, bool), mp_, np.inf)), mg)
    margin[key] = np.where(rows, mg, np.nan)
    return ok


def step(inp, ar=LD, model=None, g_allow=None):
    """One launch: inp["op"] in ("gyk", "gyf", "ahf").  Returns val (every buffer and state field after the launch),
    scale / extra (absolute error scales and additive int8 terms, same keys where defined), wrote (row masks of what
    the launch writes per buffer), state / flags (dicts), done_count, mspcount, mask, margin."""
    op = inp["op"]
    o = _Ops(inp, ar)
    m, n = o.m, o.n
    B = ar.r(inp["B"])
    b = B.shape[0]
    it = int(inp["it"])
    q = int(inp.get("q", (it - 1) & 1))
    gyf, ahf = op == "gyf", op == "ahf"
    lazy = gyf or bool(inp["lazy"])
    use_la, use_ax = gyf or bool(inp["use_la"]), gyf or bool(inp["use_ax"])
    yn_id = 0 if (op == "gyk" and inp["yn_copy"]) else 2 - q
    msp_on = gyf and bool(inp["msp"])
    ctl = bool(inp["ctl"])
    fixup = it == int(inp["maxiter"])
    fixed = bool(inp["fixed_iters"])
    tol_rel, tol_abs, rho = (ar.r(inp[k]) for k in ("tol_rel", "tol_abs", "rho"))
    S, F = _load(inp, ar)
    done_count, mspcount = int(inp["done_count"]), int(inp["mspcount"])
    buf = {k: (ar.c(inp[k]) if inp.get(k) is not None else None) for k in VEC_M + VEC_N}
    val, scale, extra, wrote, margin, mask, copied = {}, {}, {}, {}, {}, {}, {}
    none = np.zeros(b, bool)
    nanr = np.full(b, np.nan)
    zm = ar.c(np.zeros((b, m)))
    blk = np.arange(b) // 16

    def anyblk(rows):
        return np.bincount(blk, weights=rows.astype(float), minlength=blk.max() + 1)[blk] > 0

    live0 = F["done"] == 0
    act = anyblk(live0 & (F["mzit"] < it)) if gyf else np.ones(b, bool)
    mask["act"] = act
    zodd = it & 1
    Zc, Nc = buf["Zb1" if zodd else "Zb2"], buf["Nb1" if zodd else "Nb2"]
    zn_name = "Zb2" if zodd else "Zb1"
    yo_name, yn_name = f"Y{q}", f"Y{1 - q}"
    so_name, sn_name = f"S{(it + 1) & 1}", f"S{it & 1}"
    Yo = buf[yo_name]
    npv, flv = _profile(inp, b)
    g = s_g = e_g = None
    run = none
    if not ahf:
        live = act & live0
        Mi = buf["M"]
        avok = live & use_ax & (F["avok"] != 0)
        pend = live & lazy & (F["dpend"] != 0)
        ms = none.copy()
        if msp_on and it >= 2:
            ms = live & ((F["msp"] != 0) | (avok & (F["kfok"] != 0) & (F["nzero"] != 0) &
                                           np.asarray(S["opt_obj"] < ar.inf, bool) & (F["fzit"] == it - 1)))
        ent = ms & (F["msp"] == 0)
        oss, oys = np.where(live, F["optsrc"], 0), np.where(live, F["optysrc"], 0)
        mu_entry = S["mu"].copy()
        # ---- the pending convergence tests of the previous iteration (dual_finish)
        stop_in, bump_in, dpass = none.copy(), none.copy(), none.copy()
        margin["dual"], margin["bump_in"] = nanr.copy(), nanr.copy()
        if pend.any():
            Ynb = buf[yn_name]
            v0, v1 = _w(pend, Yo, zm), _w(pend, Yo - Ynb, zm)
            Kv0, Kv1 = v0 @ o.K.T, v1 @ o.K.T
            nv, dv = ar.re(_rowsum(ar.conj(v0) * Kv0)), ar.re(_rowsum(ar.conj(v1) * Kv1))
            a0, a1 = ar.cabs(v0), ar.cabs(v1)
            s1 = _w(pend, ar.cabs(Yo) + ar.cabs(Ynb), ar.cabs(zm))
            aK = ar.r(o.absK)
            scale["nAtY_in"] = _rowsum(a0 * ar.cabs(Kv0))
            scale["dAtY_in"] = _rowsum(s1 * ar.cabs(Kv1) + a1 * (s1 @ aK.T) + a1 * ar.cabs(Kv1))
            extra["nAtY_in"] = _rowsum(a0 * ar.r(o.i8(o.EK, o.c2, v0, Kv0)))
            extra["dAtY_in"] = _rowsum(a1 * ar.r(o.i8(o.EK, o.c2, v1, Kv1)))
            mu = S["mu"]
            rd = mu * ar.sqrt(ar.fmax0(dv) + S["pd_dZ2"])
            td = tol_abs * ar.sqrt(ar.r(2 * n)) + tol_rel * ar.sqrt(ar.fmax0(nv) + S["pd_nZ2"])
            dpass = pend & np.asarray(rd < td, bool)
            stop_in = dpass & (not fixed)
            cont = pend & ~stop_in
            bump_in = cont & np.asarray(S["pd_rc"] > S["last_res"] * ar.r(0.9), bool)
            margin["dual"] = np.where(pend, _rel(ar, rd, td), np.nan)
            margin["bump_in"] = np.where(cont, _rel(ar, S["pd_rc"], S["last_res"] * ar.r(0.9)), np.nan)
            S["dAtY"], S["nAtY"] = _w(pend, dv, S["dAtY"]), _w(pend, nv, S["nAtY"])
            val["res_dual"], val["t_dual"] = rd, td
            F["dpend"] = np.where(pend, 0, F["dpend"])
            F["status"] = np.where(dpass, F["status"] | ST_CONVERGED, F["status"])
            F["done"] = np.where(stop_in, 1, F["done"])
            done_count += int(stop_in.sum())
            S["mu"] = _w(bump_in, mu * rho, mu)
            S["last_res"] = _w(cont, S["pd_rc"], S["last_res"])
        mask.update(pend_in=pend, stop_in=stop_in, bump_in=bump_in, dual_pass=dpass)
        run = live & ~stop_in
        # ---- deferred opt_Y: saved before the Y-step overwrites its buffer (decided on the state at entry)
        sv = live & (yn_id != 0) & (oys == yn_id)
        if sv.any():
            buf["optY"] = _w(sv, buf[yn_name], buf["optY"] if buf["optY"] is not None else zm)
        copied["optY"] = sv.copy()
        # ---- T = (Y - M/mu) - A V
        mu = S["mu"]
        muT = mu_entry if model == "stale_mu" else mu
        imu = (1 / muT)[:, None]
        SY = Yo - Mi * imu
        e_T = np.zeros((b, m))
        la_rows = run & ~avok & use_la
        AV = zm.copy()
        if avok.any():
            AV = _w(run & avok, buf["AX"], AV)
        if la_rows.any():
            nz = (F["nzero"] != 0)
            Nn_ = _w(nz, Zc * 0, Nc if Nc is not None else Zc * 0)
            V = _w(la_rows, Zc - Nn_ * imu, Zc * 0)
            AVl = V @ o.A.T
            AV = _w(la_rows, AVl, AV)
            e_T = np.where(la_rows[:, None], o.i8(o.EA, o.c, V, AVl, bound=ar.f64(S["vbound"])), 0.0)
        T = SY - AV
        s_T = ar.cabs(Yo) + ar.cabs(Mi) * imu + ar.cabs(AV)
        given = run & ~avok & (not use_la)
        if given.any():
            T = _w(given, buf["T"], T)
            s_T = _w(given, ar.cabs(buf["T"]), s_T)
        T = _w(run, T, zm)
        # ---- g = G T, the Y-step, the sums
        g = T @ o.G.T
        aG = ar.cabs(o.G)
        s_g = _w(run, s_T, ar.cabs(zm)) @ aG.T
        e_g = ar.r(e_T) @ aG.T
        if g_allow is not None:              # (the n-space comparison: G against the exact inverse, the inputs' own errors)
            e_g = e_g + ar.r(g_allow)
        s_ge = s_g + e_g / ar.r(TOL_MULT * U)
        ys = ystep(ar, Yo, Mi, B, g, muT, s_ge)
        Yn_, Mn_, ax = ys["Y"], ys["M"], ys["ax"]
        sums = {k: ys[k] for k in ("obj2", "nAX2", "nY2", "nJM2", "dY2")}
        if model == "no_zero_guard":
            zg = np.asarray(ar.cabs(ax + Mi * imu) == 0, bool)
            Yn_ = np.where(zg, np.nan, Yn_)
            for k in sums:
                sums[k] = np.where(zg.any(axis=1), np.nan, sums[k])
        mp_ = (m + 31) & ~31
        if model == "pad_in_sums" and mp_ > m:      # rows m .. mp - 1 as a kernel without `i < m`: the clamped loads
            pc = np.full(mp_ - m, m - 1)
            yp = ystep(ar, Yo[:, pc], Mi[:, pc], B[:, pc], g[:, pc] * 0, muT)
            for k in sums:
                sums[k] = sums[k] + yp[k]
        sc = ys["scale"]
        mask["zero_guard"] = run & np.asarray(ar.cabs(ax + Mi * imu) == 0, bool).any(axis=1)
        for k, v, s_ in (("M", Mn_, sc["M"]), (yn_name, Yn_, sc["Y"])):
            buf[k] = _w(run, v, buf[k] if buf[k] is not None else zm)
            scale[k], wrote[k] = s_, run.copy()
        if use_ax:
            buf["AX"] = _w(run, ax, buf["AX"] if buf["AX"] is not None else zm)
            scale["AX"], wrote["AX"] = ar.cabs(Yo) + ar.cabs(Mi) * imu + s_ge, run.copy()
        if not gyf:
            buf["g"] = _w(run, g, buf["g"] if buf["g"] is not None else zm)
            scale["g"], wrote["g"] = s_ge, run.copy()
        val["T"], scale["T"], extra["T"] = T, s_T, e_T
        val["g_"], scale["g_"] = g, s_ge
        # ---- m-space candidates: the two sums, S' = S + g, the deferred opt_S
        cand = ms & run
        v7 = v8 = s_v7 = s_v8 = ar.r(np.zeros(b))
        if cand.any():
            kg = T - g
            a_g, a_av, a_kg = ar.cabs(g), ar.cabs(AV), ar.cabs(kg)
            v7 = ar.re(_rowsum(ar.conj(AV) * g))
            v8 = ar.re(_rowsum(ar.conj(g) * kg)) if model != "fs3_from_gg" else _rowsum(ar.abs2(g))
            s_az = 2 * s_T + ar.r(e_T) / ar.r(TOL_MULT * U)
            s_v7 = _rowsum(s_az * a_g + a_av * s_ge + a_av * a_g)
            s_v8 = _rowsum(s_ge * a_kg + a_g * (s_T + s_ge + a_kg) + a_g * a_kg)
            Sold = buf[so_name] if buf[so_name] is not None else zm
            keep_old = cand if model == "S_not_reset" else cand & ~ent
            Sn_ = _w(keep_old, Sold, zm) + g
            dso = cand & (oss == 4 + (it & 1))
            if dso.any():
                buf["optS"] = _w(dso, buf[sn_name], buf["optS"] if buf["optS"] is not None else zm)
            copied["optS"] = dso
            buf[sn_name] = _w(cand, Sn_, buf[sn_name] if buf[sn_name] is not None else zm)
            scale[sn_name], wrote[sn_name] = _w(keep_old, ar.cabs(Sold), ar.cabs(zm)) + s_ge + ar.cabs(Sn_), cand.copy()
        mask.update(run=run, cand=cand, ent=ent & run, avok=avok, la_rows=la_rows)
        # ---- the control block
        obj = ar.sqrt(sums["obj2"])
        imp = run & np.asarray(obj < S["opt_obj"], bool)
        margin["improved"] = np.where(run, _rel(ar, obj, S["opt_obj"]), np.nan)
        for k in sums:
            S[k] = _w(run, sums[k], S[k])
            scale[k] = sc[k]
        if yn_id:
            imp_id = (q + 1) if model == "optY_from_Yo" else yn_id
            F["optysrc"] = np.where(run, np.where(imp, imp_id, np.where(oys == yn_id, 0, oys)), F["optysrc"])
        else:
            src = Yo if model == "optY_from_Yo" else Yn_
            buf["optY"] = _w(imp, src, buf["optY"] if buf["optY"] is not None else zm)
            scale["optY"], wrote["optY"] = sc["Y"], imp.copy()
        take = none.copy()
        margin["entry"] = nanr.copy()
        if cand.any():
            two = 1 if model == "fs0_no_2" else 2
            s0 = S["fs0"] + two * v7 + v8
            s3 = v8
            s_s0 = abs(S["fs0"]) + 2 * s_v7 + s_v8
            room = ar.r(1.0 if model == "kfcum_no_room" else inp["room"])
            cum_e = S["kfcum"] + room * ar.sqrt(ar.fmax0(s3))
            okb = _bound(ar, S, s0, cum_e, npv, flv, cand & ent, margin, "entry")
            take = cand & (~ent | okb)
            mspcount += int(take.sum())
            S["fs0"], S["fs3"] = _w(take, s0, S["fs0"]), _w(take, s3, S["fs3"])
            scale["fs0"], scale["fs3"] = s_s0, s_v8
            F["fzit"], F["mzit"] = np.where(take, it, F["fzit"]), np.where(take, it, F["mzit"])
            te = take & ent
            F["msp"] = np.where(te, 1, F["msp"])
            F["z0id"] = np.where(te, 1 if zodd else 2, F["z0id"])
            F["msp_pad"] = np.where(te, it, F["msp_pad"])
            F["optsrc"] = np.where(cand & (oss == 4 + (it & 1)), 3, F["optsrc"])
        mask.update(imp=imp, take=take)
        if (take & ctl & (not fixup)).any():
            done_count = _fused_control(ar, inp, S, F, take, it, m, n, npv, flv, scale, margin, mask, done_count, msp_on)
        # ---- K Y' and the dual terms
        if not lazy:
            Yl = _w(run, Yn_, zm)
            KY = Yl @ o.K.T
            e_KY = o.i8(o.EK, o.c2, Yl, KY)
            s_KY = sc["Y"] @ ar.r(o.absK).T + ar.cabs(KY)
            KYo = buf[f"KY{q}"]
            dy, dk = Yl - Yo, KY - KYo
            dAtY = ar.re(_rowsum(ar.conj(dy) * dk))
            nAtY = ar.re(_rowsum(ar.conj(Yl) * KY))
            S["dAtY"], S["nAtY"] = _w(run, dAtY, S["dAtY"]), _w(run, nAtY, S["nAtY"])
            a_dy, a_dk = ar.cabs(dy), ar.cabs(dk)
            scale["dAtY"] = _rowsum((sc["Y"] + ar.cabs(Yo)) * a_dk + a_dy * (s_KY + ar.cabs(KYo)) + a_dy * a_dk)
            scale["nAtY"] = _rowsum(sc["Y"] * ar.cabs(KY) + ar.cabs(Yl) * s_KY + ar.cabs(Yl) * ar.cabs(KY))
            extra["dAtY"], extra["nAtY"] = _rowsum(a_dy * ar.r(e_KY)), _rowsum(ar.cabs(Yl) * ar.r(e_KY))
            buf[f"KY{1 - q}"] = _w(run, KY, buf[f"KY{1 - q}"] if buf[f"KY{1 - q}"] is not None else zm)
            scale[f"KY{1 - q}"], extra[f"KY{1 - q}"], wrote[f"KY{1 - q}"] = s_KY, e_KY, run.copy()
    # ---- the fused apply_AH pass (gyf_kernel's second half, or the stand-alone FUSE kernel)
    if gyf or ahf:
        if ahf:
            g = ar.c(inp["g"])
            s_ge = ar.cabs(g) * 0
            act = np.ones(b, bool)
        za_msp = msp_on
        P_ = act & (F["done"] == 0) & ~(za_msp & (F["mzit"] == it))
        el = P_ & (F["kfok"] != 0) & (F["nzero"] != 0)
        obj_n = ar.sqrt(S["obj2"])
        imp_pre = np.asarray(obj_n < S["opt_obj"], bool)
        keep_cur = el & ~imp_pre & ~np.asarray(S["opt_obj"] < ar.inf, bool)
        gl = _w(P_, g, g * 0)
        W = gl @ ar.conj(o.A)
        e_W = o.i8(o.EAH, o.c, gl, W)
        s_W = _w(P_, s_ge + ar.cabs(g), s_ge * 0) @ ar.r(o.absA) + ar.cabs(W)
        zn_id = 1 + (it & 1)
        zn = ar.c(np.zeros((b, n)))
        sv = el & (F["optsrc"] == zn_id)
        if sv.any():
            buf["optX"] = _w(sv, buf[zn_name], buf["optX"] if buf["optX"] is not None else zn)
            F["optsrc"] = np.where(sv, 0, F["optsrc"])
        copied["optX"] = sv
        Zl = _w(el, Zc, zn) if Zc is not None else zn
        Xn_ = Zl + W
        buf[zn_name] = _w(el, Xn_, buf[zn_name] if buf[zn_name] is not None else zn)
        s_X = ar.cabs(Zl) + s_W + ar.cabs(Xn_)
        scale[zn_name], extra[zn_name], wrote[zn_name] = s_X, e_W, el.copy()
        buf["Xcur"] = _w(keep_cur, Xn_, buf["Xcur"] if buf["Xcur"] is not None else zn)
        scale["Xcur"], extra["Xcur"], wrote["Xcur"] = s_X, e_W, keep_cur
        ne = P_ & ~el
        buf["X"] = _w(ne, W, buf["X"] if buf["X"] is not None else zn)
        scale["X"], extra["X"], wrote["X"] = s_W, e_W, ne
        f0, f3 = _rowsum(ar.abs2(Xn_)), _rowsum(ar.abs2(W))
        a_x, a_w = ar.cabs(Xn_), ar.cabs(W)
        # ||X||^2 and ||X - Z||^2: the kernel forms d = fl(Z + W) - Z, within u |X| of W
        sc0 = _rowsum(2 * a_x * s_X + a_x * a_x)
        sc3 = _rowsum(2 * a_w * (s_W + a_x) + a_w * a_w)
        ex0, ex3 = _rowsum(2 * a_x * ar.r(e_W)), _rowsum(2 * a_w * ar.r(e_W))
        S["fs0"], S["fs3"] = _w(el, f0, S["fs0"]), _w(el, f3, S["fs3"])
        scale["fs0"] = _w(el, sc0, scale.get("fs0", sc0 * 0))
        scale["fs3"] = _w(el, sc3, scale.get("fs3", sc3 * 0))
        extra["fs0"], extra["fs3"] = _w(el, ex0, ex0 * 0), _w(el, ex3, ex3 * 0)
        F["fzit"] = np.where(el, it, F["fzit"])
        mask.update(ah=P_, el=el, keep_cur=keep_cur, ah_save=sv)
    for k in VEC_M + VEC_N:
        val[k] = buf[k]
        wrote.setdefault(k, none.copy())
        copied.setdefault(k, none.copy())
    return dict(val=val, scale=scale, extra=extra, wrote=wrote, copied=copied, state=S, flags=F, done_count=done_count,
                mspcount=mspcount, mask=mask, margin=margin)


def _fused_control(ar, inp, S, F, take, it, m, n, npv, flv, scale, margin, mask, done_count, za_msp):
    """fused_control<false> -> iter_control_in (lazy form) -> the deferral of the best iterate, on the rows `take`."""
    tiny = ar.r(1e-300)
    tol_rel, tol_abs, rho = (ar.r(inp[k]) for k in ("tol_rel", "tol_abs", "rho"))
    fixed = bool(inp["fixed_iters"])
    s0, s3 = S["fs0"], S["fs3"]
    rs3 = ar.sqrt(ar.fmax0(s3))
    cum = (S["kfcum"] + rs3) * ar.r(1.0 + 2.0 ** -40)
    ok = _bound(ar, S, s0, cum, npv, flv, take, margin, "bound")
    ok = ok & ~(za_msp & (F["mzit"] == it) & (it == int(inp["msp_fail_it"])))
    ps = take & ok
    mask["ctl"], mask["bound_fail"] = ps, take & ~ok
    obj = ar.sqrt(S["obj2"])
    imp_pre = ps & np.asarray(obj < S["opt_obj"], bool)
    optsrc0 = F["optsrc"].copy()
    nX = ar.sqrt(s0)
    nAX, nY = ar.sqrt(S["nAX2"]), ar.sqrt(S["nY2"])
    rp = ar.sqrt(S["nJM2"])
    rc2 = rp * rp + S["dY2"] + s3
    rc = ar.sqrt(rc2)
    s_rc = (scale["nJM2"] + scale["dY2"] + scale["fs3"]) / (2 * rc + tiny) + rc
    mx1 = ar.fmax(nAX, nY)
    tp = tol_abs * ar.sqrt(ar.r(m + n)) + tol_rel * ar.sqrt(mx1 * mx1 + nX * nX)
    tc = tol_abs * ar.sqrt(ar.r(2 * (m + n))) + tol_rel * ar.sqrt(mx1 * mx1 + nX * nX + nY * nY + nX * nX)
    P, Cc = np.asarray(rp < tp, bool), np.asarray(rc < tc, bool)
    pendn = ps & P & ~Cc
    conv = ps & ~pendn & Cc
    stop = conv & (not fixed)
    upd = ps & ~pendn & ~stop
    bump = upd & np.asarray(rc > S["last_res"] * ar.r(0.9), bool)
    margin["primal"] = np.where(ps, _rel(ar, rp, tp), np.nan)
    margin["combined"] = np.where(ps, _rel(ar, rc, tc), np.nan)
    margin["bump"] = np.where(upd, _rel(ar, rc, S["last_res"] * ar.r(0.9)), np.nan)
    mask.update(pendn=pendn, conv=conv, stop=stop, bump=bump, imp_ctl=imp_pre)
    S["opt_obj"] = _w(imp_pre, obj, S["opt_obj"])
    scale["opt_obj"] = scale["obj2"] / (2 * obj + tiny) + obj
    F["iters"] = np.where(ps, it, F["iters"])
    F["dpend"] = np.where(pendn, 1, F["dpend"])
    S["pd_dZ2"], S["pd_nZ2"], S["pd_rc"] = _w(pendn, s3, S["pd_dZ2"]), _w(pendn, nX * nX, S["pd_nZ2"]), _w(pendn, rc, S["pd_rc"])
    scale["pd_dZ2"], scale["pd_nZ2"], scale["pd_rc"] = scale["fs3"], scale["fs0"] + 2 * abs(s0), s_rc
    F["status"] = np.where(conv, F["status"] | ST_CONVERGED, F["status"])
    F["done"] = np.where(stop, 1, F["done"])
    done_count += int(stop.sum())
    S["mu"] = _w(bump, S["mu"] * rho, S["mu"])
    S["last_res"] = _w(upd, rc, S["last_res"])
    scale["last_res"] = s_rc
    S["vbound"] = _w(ps, nX * ar.r(1.0 + 2.0 ** -40), S["vbound"])
    scale["vbound"] = scale["fs0"] / (2 * nX + tiny) + nX
    F["nzero"], F["avok"] = np.where(ps, 1, F["nzero"]), np.where(ps, 1, F["avok"])
    mz = za_msp & (F["mzit"] == it)
    F["optsrc"] = np.where(ps, np.where(imp_pre, np.where(mz, 4 + (it & 1), 1 + (it & 1)), optsrc0), F["optsrc"])
    S["kfcum"] = _w(ps, cum, S["kfcum"])
    scale["kfcum"] = scale["fs3"] / (2 * rs3 + tiny) + abs(cum)
    F["zit"] = np.where(ps, it, F["zit"])
    return done_count


# ---------------------------------------------------------------- packing
def pack_state(S, ar=LD):
    return np.stack([ar.f64(S[k]).astype(np.float64) for k in STATE], axis=1)


def pack_flags(Fl):
    return np.stack([np.asarray(Fl[k]) for k in FLAGS], axis=1).astype(np.int32)


def chain_input(inp, ref, ar=LD, **over):
    """The next launch's inputs from a reference result (rounded to f64, as the state passes through the host)."""
    out = dict(inp)
    for k in VEC_M + VEC_N:
        out[k] = None if ref["val"][k] is None else ar.f64(ref["val"][k])
    out.update(state=pack_state(ref["state"], ar), flags=pack_flags(ref["flags"]), done_count=ref["done_count"],
               mspcount=ref["mspcount"])
    out.update(over)
    out.pop("q", None)
    return out


# ---------------------------------------------------------------- msr_kernel: k iterations in one launch
def run(inp, ar=LD, model=None, stepper=None):
    """launch_msr from iteration inp["it"] to inp["it_end"] - 1: gyf's m-space iteration chained per 16-realisation
    block with msr_kernel's entry checks, stop rules, write-back positions and counters.  Best iterates come back
    resolved as the run leaves them (opt_Y / opt_S written, optysrc 0 / optsrc 3).  Returns step's dict of the last
    state plus resume, steps [4], vecw."""
    it0, it_end = int(inp["it"]), int(inp["it_end"])
    S, F = _load(inp, ar)
    b = len(F["done"])
    nblk = (b + 15) // 16
    cur = dict(inp, op="gyf", msp=1, ctl=1, use_la=1, use_ax=1, lazy=1)
    cur.pop("q", None)
    resume, steps, vecw = it_end, [0, 0, 0, 0], 0
    blk = np.arange(b) // 16
    live = F["done"] == 0
    go = np.zeros(b, bool)
    for k in range(nblk):
        r = blk == k
        lv = r & live
        if (lv & (F["mzit"] >= it0)).any():
            resume = min(resume, int(F["mres"][lv & (F["mzit"] >= it0)].min()))
            continue
        bad = lv & ((F["msp"] == 0) | (F["dpend"] != 0) | (F["mzit"] != it0 - 1) | (F["zit"] != it0 - 1))
        if bad.any():
            resume = min(resume, it0)
            steps[1] += 1
            continue
        go |= lv
    # the deferred best iterates of the rows that run are flushed first
    bufs = {k: (None if inp.get(k) is None else np.array(inp[k], np.complex128)) for k in VEC_M + VEC_N}
    st, fl = np.array(inp["state"], np.float64), np.array(inp["flags"], np.int32)
    fi = {k: i for i, k in enumerate(FLAGS)}
    for j in np.nonzero(go)[0]:
        oy, os_ = fl[j, fi["optysrc"]], fl[j, fi["optsrc"]]
        if oy in (1, 2):
            bufs["optY"][j] = bufs[f"Y{oy - 1}"][j]
            fl[j, fi["optysrc"]] = 0
            vecw += 1
        if os_ in (4, 5):
            bufs["optS"][j] = bufs[f"S{os_ - 4}"][j]
            fl[j, fi["optsrc"]] = 3
            vecw += 1
    cur.update(bufs, state=st, flags=fl)
    # rows that do not run are hidden from the chained steps (done) and restored at the end
    hide = ~go & (fl[:, fi["done"]] == 0)
    stopped_blk = np.zeros(nblk, bool) | ~np.array([(go & (blk == k)).any() for k in range(nblk)])
    res = None
    pbY, pbS = np.zeros(b, bool), np.zeros(b, bool)
    mres = fl[:, fi["mres"]].copy()
    dead = np.zeros(b, bool)
    it = it0
    while not stopped_blk.all():
        f2 = np.array(cur["flags"], np.int32)
        frozen = hide | (np.repeat(stopped_blk, 16)[:b] & (f2[:, fi["done"]] == 0))
        f2[frozen, fi["done"]] = 1
        if stepper is not None:          # (the GPU test: one gyf launch per iteration in place of the reference's step)
            res = stepper(dict(cur, flags=f2, it=it))
        else:
            res = step(dict(cur, flags=f2, it=it), ar, model if model in ("fs0_no_2", "fs3_from_gg", "stale_mu") else None)
        rn = res["mask"]["run"]
        ok = res["mask"].get("ctl", np.zeros(b, bool))
        imp = res["mask"]["imp"]
        pendn = res["mask"].get("pendn", np.zeros(b, bool))
        nf = pack_flags(res["flags"])
        nf[frozen, fi["done"]] = 0
        # best iterates: written when the next iterate does not beat them, or at the write-back
        vecw += int((rn & pbY & ~imp).sum()) + int((rn & pbS & ~imp).sum())
        pbY = np.where(rn, imp, pbY)
        pbS = np.where(rn, imp & ok, pbS)
        steps[0] += int(rn.sum())
        nxt = chain_input(cur, res, ar, flags=nf)
        nxt["mspcount"] = res["mspcount"]
        for k in range(nblk):
            r = (blk == k) & rn
            if stopped_blk[k] or not r.any():
                continue
            fail, pnd = (r & ~ok).any(), (r & pendn).any()
            alive = (r & (nf[:, fi["done"]] == 0)).any()
            stop = fail or pnd or it + 1 >= it_end or not alive
            wbrows = r & ((nf[:, fi["done"]] != 0) | stop)
            vecw += int(6 * wbrows.sum() + (wbrows & pbY).sum() + (wbrows & pbS).sum())
            if stop:
                # an improving iterate whose bound failed: the Z-step of `it` records X itself, and the run leaves
                # opt_S as it stands (nothing reads it before that Z-step overwrites optsrc)
                dead |= r & imp & ~ok
                rp = it if fail else it + 1
                if model == "resume_plus1":
                    rp = it + 1
                stopped_blk[k] = True
                lvr = r & (nf[:, fi["done"]] == 0)
                mres[lvr] = rp
                if alive:
                    resume = min(resume, rp)
                if fail or pnd:
                    steps[2 if fail else 3] += 1
        cur = nxt
        it += 1
    out = res if res is not None else step(dict(cur, flags=np.where(np.arange(len(FLAGS)) == fi["done"], 1, fl), it=it0), ar)
    fin_f = np.array(cur["flags"], np.int32)
    fin_s = np.array(cur["state"], np.float64)
    # resolve the deferrals of the chained gyf steps the way the run leaves them
    vals = {k: (None if cur.get(k) is None else np.array(cur[k])) for k in VEC_M + VEC_N}
    for j in np.nonzero(go)[0]:
        oy, os_ = fin_f[j, fi["optysrc"]], fin_f[j, fi["optsrc"]]
        if oy in (1, 2):
            vals["optY"][j] = vals[f"Y{oy - 1}"][j]
            fin_f[j, fi["optysrc"]] = 0
        if os_ in (4, 5):
            vals["optS"][j] = vals[f"S{os_ - 4}"][j]
            fin_f[j, fi["optsrc"]] = 3
    fin_f[:, fi["mres"]] = mres
    if model == "wb_parity":
        for a_, b_ in (("Y0", "Y1"), ("S0", "S1")):
            x, y = vals[a_].copy(), vals[b_].copy()
            vals[a_][go], vals[b_][go] = y[go], x[go]
    return dict(val=vals, state=fin_s, flags=fin_f, done_count=int(cur["done_count"]), mspcount=int(cur["mspcount"]),
                resume=resume, steps=steps, vecw=vecw, ran=go, last=out, it_last=it - 1, dead_optS=dead)


def ready(flags, it):
    """launch_msr_ready: the three counts."""
    f = {k: np.asarray(flags)[:, i] for i, k in enumerate(FLAGS)}
    lv = f["done"] == 0
    bad = lv & ((f["msp"] == 0) | (f["dpend"] != 0) | (f["mzit"] < it - 1) | (f["zit"] < it - 1))
    # the diagnostics are added only by the 256-realisation groups that have a realisation not ready
    nm, np_ = lv & (f["msp"] == 0), lv & (f["dpend"] != 0)
    grp = np.arange(len(lv)) // 256
    hit = np.bincount(grp, weights=bad.astype(float))[grp] > 0
    return [int(bad.sum()), int((nm & hit).sum()), int((np_ & hit).sum())]


def optx(inp, ar=LD):
    """launch_i8_msp_optx: opt_S gathered from S0 / S1 (optsrc 4 / 5), then opt_X = Z0 + c A^H opt_S where optsrc is 3."""
    o = _Ops(inp, ar)
    S, F = _load(inp, ar)
    b = len(F["done"])
    zm, zn = ar.c(np.zeros((b, o.m))), ar.c(np.zeros((b, o.n)))
    optS = ar.c(inp["optS"]) if inp.get("optS") is not None else zm
    for k, name in ((4, "S0"), (5, "S1")):
        r = F["optsrc"] == k
        if r.any():
            optS = _w(r, ar.c(inp[name]), optS)
    gathered = (F["optsrc"] == 4) | (F["optsrc"] == 5)
    rows = gathered | (F["optsrc"] == 3)
    gl = _w(rows, optS, zm)
    W = gl @ ar.conj(o.A)
    e_W = o.i8(o.EAH, o.c, gl, W)
    Z0 = _w(F["z0id"] == 1, ar.c(inp["Zb1"]), ar.c(inp["Zb2"]))
    X = _w(rows, Z0, zn) + W
    return dict(optX=X, optS=optS, rows=rows, gathered=gathered, scale=ar.cabs(_w(rows, Z0, zn)) + 2 * ar.cabs(W),
                extra=e_W, optsrc=np.where(rows, 0, F["optsrc"]))


# ---------------------------------------------------------------- (a) the n-space truth
def _oracle():
    p = str(pathlib.Path(__file__).resolve().parents[1] / "oracle")
    if p not in sys.path:
        sys.path.insert(0, p)
    import ace_oracle
    return ace_oracle


def nspace_step(inp, mu=None):
    """One InferADMM A2only iteration in longdouble on explicit n-vectors, for the realisations a gyk / gyf launch
    iterates: Z = the Z buffer of the previous iterate, or Z0 + A^H S for a realisation in m-space form; V = Z - N/mu
    (N = 0 where it is held as zero).  mu: the penalty the iteration runs with where it is not the state's (a pending
    test finished first).  Returns X, AX, Y', M', g*, the sums, ||X||^2, ||X - Z||^2, dG = ||G - (I + K)^-1||_inf and
    what the inputs disagree by (AX_in against A V, fs0_in against ||Z||^2).  For the stand-alone fused apply_AH only
    X = Z + A^H g of the caller's g, with the caller's A as it stands, ||X||^2 and ||X - Z||^2."""
    ar = LD
    it = int(inp["it"])
    if inp["op"] == "ahf":
        Zc, g = ar.c(inp["Zb1" if it & 1 else "Zb2"]), ar.c(inp["g"])
        W = g @ ar.conj(ar.c(inp["A"]))
        X = Zc + W
        return dict(X=X, W=W, Z=Zc, fs0=_rowsum(ar.abs2(X)), fs3=_rowsum(ar.abs2(W)), dG=0.0, kappa=1.0)
    O = _oracle()
    o = _Ops(inp, ar)
    S, F = _load(inp, ar)
    if mu is not None:
        S["mu"] = ar.r(mu)
    q = int(inp.get("q", (it - 1) & 1))
    B = ar.r(inp["B"])
    b = B.shape[0]
    Yo, M = ar.c(inp[f"Y{q}"]), ar.c(inp["M"])
    Zc = ar.c(inp["Zb1" if it & 1 else "Zb2"])
    inform = F["msp"] != 0
    Z = Zc
    if inform.any():
        Z0 = _w(F["z0id"] == 1, ar.c(inp["Zb1"]), ar.c(inp["Zb2"]))
        Sold = ar.c(inp[f"S{(it + 1) & 1}"])
        Z = _w(inform, Z0 + _w(inform, Sold, Sold * 0) @ ar.conj(o.A), Zc)
    mu = S["mu"][:, None]
    Nc = inp.get("Nb1" if it & 1 else "Nb2")
    Nn = _w(F["nzero"] != 0, Z * 0, ar.c(Nc) if Nc is not None else Z * 0)
    V = Z - Nn / mu
    AV = V @ o.A.T
    T = (Yo - M / mu) - AV
    K64 = F64.c(ar.f64(o.K))
    gs, kappa, Binv = L.g_reference(K64, F64.c(ar.f64(T)))
    # (g_reference takes T rounded to f64; the residual of that rounding is solved to first order with its f64 inverse)
    gs = gs + ar.c((T - ar.c(F64.c(ar.f64(T)))) @ ar.c(Binv).T)
    X = V + gs @ ar.conj(o.A)
    AX = X @ o.A.T
    Yn = np.empty_like(AX)
    for j in range(b):      # ArgMinY :511-533, column mode at r = 1, through the oracle
        Yn[j] = O.argmin_y(AX[j][:, None].copy(), B[j], M[j][:, None], S["mu"][j], False)[:, 0]
    JM = AX - Yn
    Mn = M + mu * JM
    aax = ar.cabs(AX) - B
    dG = L.ninf(F64.c(ar.f64(o.G)) - Binv)
    return dict(X=X, AX=AX, Yn=Yn, M=Mn, g=gs, T=T, Z=Z, obj2=_rowsum(aax * aax), nAX2=_rowsum(ar.abs2(AX)),
                nY2=_rowsum(ar.abs2(Yn)), nJM2=_rowsum(ar.abs2(JM)), dY2=_rowsum(ar.abs2(Yn - Yo)),
                fs0=_rowsum(ar.abs2(X)), fs3=_rowsum(ar.abs2(X - Z)), dG=dG, kappa=kappa,
                e_AX=ar.cabs(ar.c(inp["AX"]) - AV) if inp.get("AX") is not None else None,
                e_fs0=abs(S["fs0"] - _rowsum(ar.abs2(Z))), Tinf=np.max(ar.cabs(T), axis=1))


def truth_allowance(inp, tr):
    """The n-space comparison's additive term on g per realisation: ||G - (I + K)^-1||_inf ||T||_inf, plus
    |G| applied to the inputs' own inconsistency (the stored AX against A Z)."""
    ar = LD
    aG = ar.cabs(ar.c(inp["G"]))
    e = (ar.r(tr["dG"]) * tr["Tinf"])[:, None] + 0 * ar.cabs(tr["g"])
    if tr["e_AX"] is not None:
        S, F = _load(inp, ar)
        e = e + _w(F["avok"] != 0, tr["e_AX"], tr["e_AX"] * 0) @ aG.T
    return e


# ---------------------------------------------------------------- comparisons (the GPU test's and the models')
def _ratio(got, ref, scale, extra, rows, mult=None):
    got = np.asarray(got)[rows]
    if not got.size:
        return 0.0
    cplx = np.iscomplexobj(got) or np.iscomplexobj(np.asarray(ref))
    got = got.astype(np.clongdouble if cplx else np.longdouble)
    ref = np.asarray(ref)[rows].astype(got.dtype)
    ex = np.asarray(extra, np.longdouble)[rows] if np.ndim(extra) else extra
    tol = tolerance(np.asarray(scale)[rows], ex) if mult is None else mult * U * np.asarray(scale, np.longdouble)[rows]
    err = np.abs(got - ref)
    both_nan = np.isnan(got) & np.isnan(ref)
    with np.errstate(all="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    ratio = np.where(both_nan, 0.0, np.where(np.isnan(ratio), np.inf, ratio))
    return float(ratio.max())


def compare_step(res, inp, ref=None, mult=None):
    """A launch's result `res` (anything with .vec / .state / .flags / .done_count / .mspcount, as ustep.UnitResult)
    against (b).  Returns (ratios: [(output, worst err / tol)], broken: [names of exact comparisons that fail], ref)."""
    ref = step(inp) if ref is None else ref
    ratios, broken = [], []
    b = np.asarray(inp["B"]).shape[0]
    allr = np.ones(b, bool)
    for k in VEC_M + VEC_N:
        w = ref["wrote"][k]
        if w.any():
            ratios.append((k, _ratio(res.vec[k], ref["val"][k], ref["scale"][k], ref["extra"].get(k, 0.0), w, mult)))
        cp = ref["copied"][k] & ~w
        if cp.any():
            a_, b_ = np.ascontiguousarray(res.vec[k][cp]), np.ascontiguousarray(F64.c(LD.f64(ref["val"][k]))[cp])
            if not np.array_equal(a_.view(np.uint64), b_.view(np.uint64)):
                broken.append(k + " (rows saved before their buffer is overwritten)")
        keep = ~w & ~cp
        if inp.get(k) is not None and keep.any():
            a_, b_ = np.ascontiguousarray(res.vec[k][keep]), np.ascontiguousarray(np.asarray(inp[k], np.complex128)[keep])
            if not np.array_equal(a_.view(np.uint64), b_.view(np.uint64)):
                broken.append(k + " (rows the launch must leave)")
    st_in = np.asarray(inp["state"], np.float64)
    for i, k in enumerate(STATE):
        rv = ref["state"][k]
        changed = LD.f64(rv).astype(np.float64) != st_in[:, i]
        changed |= np.isnan(LD.f64(rv).astype(np.float64)) != np.isnan(st_in[:, i])
        if changed.any():
            key = k if k in ref["scale"] else {"dAtY": "dAtY_in", "nAtY": "nAtY_in"}.get(k, k)
            if k in ("dAtY", "nAtY") and k not in ref["scale"]:
                key = k + "_in"
            if k == "mu" or key not in ref["scale"]:      # mu rho and values handed on: exactly
                if not np.array_equal(res.state[changed, i], LD.f64(rv).astype(np.float64)[changed]):
                    broken.append(k)
            else:
                ratios.append((k, _ratio(res.state[:, i], rv, ref["scale"][key], ref["extra"].get(key, 0.0), changed, mult)))
        same = ~changed
        if same.any() and not np.array_equal(res.state[same, i].view(np.uint64), st_in[same, i].view(np.uint64)):
            broken.append(k + " (rows the launch must leave)")
    rf = pack_flags(ref["flags"])
    for i, k in enumerate(FLAGS):
        if not np.array_equal(np.asarray(res.flags)[:, i], rf[:, i]):
            broken.append(k)
    if res.done_count != ref["done_count"]:
        broken.append("done_count")
    if res.mspcount != ref["mspcount"]:
        broken.append("mspcount")
    return ratios, broken, ref


def compare_truth(res, inp, rows=None):
    """The same launch against (a): Y', M', the stored AX (= A X), the five sums, fs0 = ||X||^2, fs3 = ||X - Z||^2 and,
    where the fused pass wrote it, X itself, for the realisations the launch iterated (and `rows`).  The tolerance is
    (b)'s with the allowance of ``truth_allowance`` on g (and the inputs' |fs0 - ||Z||^2| on fs0).  gyk with apply_A
    folded in, gyf, and the stand-alone fused apply_AH (X / Z', fs0, fs3 on the explicit Z)."""
    it = int(inp["it"])
    q = int(inp.get("q", (it - 1) & 1))
    b = np.asarray(inp["flags"]).shape[0]
    rows = np.ones(b, bool) if rows is None else np.asarray(rows, bool)
    zn = "Zb2" if it & 1 else "Zb1"
    if inp["op"] == "ahf":
        tr, ref = nspace_step(inp), step(inp)
        sc, ex, el, ne = ref["scale"], ref["extra"], ref["mask"]["el"] & rows, ref["mask"]["ah"] & ~ref["mask"]["el"] & rows
        out = [(zn, _ratio(res.vec[zn], tr["X"], sc[zn], ex[zn], el)), ("X", _ratio(res.vec["X"], tr["W"], sc["X"], ex["X"], ne)),
               ("fs0", _ratio(res.state[:, STATE.index("fs0")], tr["fs0"], sc["fs0"], LD.f64(ex["fs0"]), el)),
               ("fs3", _ratio(res.state[:, STATE.index("fs3")], tr["fs3"], sc["fs3"], LD.f64(ex["fs3"]), el))]
        return out, ref, tr
    mu = None
    if (np.asarray(inp["flags"])[:, FLAGS.index("dpend")] != 0).any():      # the mu the iteration runs with
        bi = step(inp)["mask"]["bump_in"]
        mu0 = np.asarray(inp["state"], np.float64)[:, 0]
        mu = np.where(bi, mu0 * np.float64(inp["rho"]), mu0)
    tr = nspace_step(inp, mu)
    ref = step(inp, g_allow=truth_allowance(inp, tr))
    run = ref["mask"]["run"] & rows
    sc, ex = ref["scale"], ref["extra"]
    out = [(f"Y{1 - q}", _ratio(res.vec[f"Y{1 - q}"], tr["Yn"], sc[f"Y{1 - q}"], 0.0, run)),
           ("M", _ratio(res.vec["M"], tr["M"], sc["M"], 0.0, run)),
           ("AX", _ratio(res.vec["AX"], tr["AX"], sc["AX"], 0.0, run))]
    for k in ("obj2", "nAX2", "nY2", "nJM2", "dY2"):
        out.append((k, _ratio(res.state[:, STATE.index(k)], tr[k], sc[k], 0.0, run)))
    take, el = ref["mask"].get("take", run & False) & rows, ref["mask"].get("el", run & False) & rows
    both = take | el
    if both.any():
        ex0 = np.where(take, LD.f64(tr["e_fs0"]).astype(np.float64), 0.0) + LD.f64(ex.get("fs0", 0.0) + 0 * tr["fs0"])
        ex3 = LD.f64(ex.get("fs3", 0.0) + 0 * tr["fs0"])
        out.append(("fs0", _ratio(res.state[:, STATE.index("fs0")], tr["fs0"], sc["fs0"], ex0, both)))
        out.append(("fs3", _ratio(res.state[:, STATE.index("fs3")], tr["fs3"], sc["fs3"], ex3, both)))
    if el.any():
        out.append((zn, _ratio(res.vec[zn], tr["X"], sc[zn], ex[zn], el)))
    return out, ref, tr


class FakeResult:
    """A reference result in the shape of ustep.UnitResult (for the models and the f64 transcription)."""

    def __init__(self, ref, ar=LD):
        self.vec = {k: (None if v is None else F64.c(ar.f64(v))) for k, v in ref["val"].items() if k in VEC_M + VEC_N}
        self.state = pack_state(ref["state"], ar) if isinstance(ref["state"], dict) else np.asarray(ref["state"])
        self.flags = pack_flags(ref["flags"]) if isinstance(ref["flags"], dict) else np.asarray(ref["flags"])
        self.done_count, self.mspcount = ref["done_count"], ref["mspcount"]
        for k in ("resume", "steps", "vecw"):
            if k in ref:
                setattr(self, k, ref[k])


def compare_run(res, inp, ref=None):
    """An m-space run's result against ``run``: the discrete outcome exactly, the last state within the tolerance of
    the last chained step (the iterates before it are the reference's own: the chain's growth is the caller's)."""
    ref = run(inp) if ref is None else ref
    broken = []
    for k in ("resume", "vecw", "done_count", "mspcount"):
        if int(getattr(res, k)) != int(ref[k]):
            broken.append(k)
    if list(np.asarray(res.steps)) != list(ref["steps"]):
        broken.append("steps")
    if not np.array_equal(np.asarray(res.flags), ref["flags"]):
        broken.append("flags")
    return broken, ref


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))


def compare_run_chain(res, inp, ch):
    """An m-space run's result against the chain `ch` of per-iteration steps with the run's stop rules (``run`` with
    the device's gyf launches as its stepper in the GPU test; the reference's own run for the wrong-run models): the
    counters equal, and bit for bit Y, M, AX, S, opt_Y, opt_S, the state and the flags of the realisations that ran
    (opt_S of an improving iterate whose bound failed left out: the run does not write it), every buffer and control
    block of the others, and every buffer that is none of the run's.  Returns the names that differ."""
    broken = []
    for k in ("resume", "vecw", "done_count", "mspcount"):
        if int(getattr(res, k)) != int(ch[k]):
            broken.append(k)
    if list(np.asarray(res.steps)) != list(ch["steps"]):
        broken.append("steps")
    ran = ch["ran"]
    for k in ("Y0", "Y1", "M", "AX", "S0", "S1", "optY", "optS"):
        rows = ran & ~ch["dead_optS"] if k == "optS" else ran
        if not _bits_equal(np.asarray(res.vec[k])[rows], np.asarray(ch["val"][k], np.complex128)[rows]):
            broken.append(k)
        if not _bits_equal(np.asarray(res.vec[k])[~ran], np.asarray(inp[k], np.complex128)[~ran]):
            broken.append(k + " (outside the run)")
    if not _bits_equal(np.asarray(res.state)[ran], np.asarray(ch["state"], np.float64)[ran]):
        broken.append("state")
    if not np.array_equal(np.asarray(res.flags)[ran], np.asarray(ch["flags"])[ran]):
        broken.append("flags")
    if not (_bits_equal(np.asarray(res.state)[~ran], np.asarray(inp["state"], np.float64)[~ran])
            and np.array_equal(np.asarray(res.flags)[~ran], np.asarray(inp["flags"])[~ran])):
        broken.append("control blocks outside the run")
    for k in VEC_N + ("T", "g", "KY0", "KY1"):
        if inp.get(k) is not None and not _bits_equal(np.asarray(res.vec[k]), np.asarray(inp[k], np.complex128)):
            broken.append(k + " (no buffer of the run)")
    return broken


def compare_run_fs0(res, inp, one, it, rows):
    """fs0 after the run's iteration `it` against ||Z0 + A^H S'||^2 formed explicitly in longdouble from the S the
    run wrote back (no m-space identity, no earlier fs0).  Every iteration of the run adds to fs0 an error within that
    iteration's tolerance, and the scales of the iterations agree to the size of a step (1e-4 here), so the bound is
    (it - it0 + 1) x the last iteration's tolerance (`one`: its reference step) plus what fs0 and S disagreed by on
    entry.  Returns the worst err / bound over `rows`."""
    ar = LD
    o = _Ops(inp, ar)
    S, F = _load(inp, ar)
    it0 = int(inp["it"])
    Z0 = _w(F["z0id"] == 1, ar.c(inp["Zb1"]), ar.c(inp["Zb2"]))
    X = Z0 + ar.c(res.vec[f"S{it & 1}"]) @ ar.conj(o.A)
    e0 = abs(S["fs0"] - _rowsum(ar.abs2(Z0 + ar.c(inp[f"S{(it0 + 1) & 1}"]) @ ar.conj(o.A))))
    tol = (it - it0 + 1) * tolerance(one["scale"]["fs0"]) + e0
    err = abs(ar.r(np.asarray(res.state)[:, STATE.index("fs0")]) - _rowsum(ar.abs2(X)))
    return float(np.max((err / tol)[rows])) if np.any(rows) else 0.0


# ---------------------------------------------------------------- inputs
SHAPES = {"m1-n1-b1": (1, 1, 1, "pmj1"), "m17-n33-b17": (17, 33, 17, "pmj"), "m121-n256-b35": (121, 256, 35, "twin"),
          "m243-n64-b16": (243, 64, 16, "pmj"), "m256-n1024-b35": (256, 1024, 35, "pmj")}
RUN_SHAPES = {"m256-n64-b16": (256, 64, 16, "pmj"), "m256-n64-b35": (256, 64, 35, "pmj")}


def _cx(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


@functools.lru_cache(maxsize=None)
def problem(seed, m, n, b, kind):
    """A codebook and a steady-state iterate per realisation: Z a rank-one channel (tx x rx, tx = the largest divisor
    of n up to sqrt(n)), Y = A Z perturbed by `eps`, M small, B the magnitudes of A Z perturbed."""
    rng = np.random.default_rng([seed, m, n, b])
    A = L.codebook(kind, m, n, seed)
    tx = max(d for d in range(1, int(np.sqrt(n)) + 1) if n % d == 0)
    Z = np.stack([np.outer(_cx(rng, n // tx), _cx(rng, tx)).reshape(-1) for _ in range(b)])
    Z *= (3.0 / np.linalg.norm(Z, axis=1))[:, None]
    return A, Z, int(rng.integers(1 << 30))


# Roles of a realisation in a mixed batch (``build(roles=...)``; j % len(roles) picks one):
#   enter    certified steady state, enters the m-space form with room           (take, control in place)
#   form     already in the form: Z = Z0 + A^H S, S in the S buffer of it - 1     (take, control in place)
#   form_d   the same with the best iterate deferred: optsrc 4 + (it & 1), optysrc = yn_id, not improving
#   refused  certified, but no room for 32 more steps: the plain fused pass (eligible)
#   fused    certified, the previous iteration was not a fused one (fzit = it - 2): fused pass, no candidate
#   fused_ox the same with the best X deferred in the Z' buffer this pass overwrites (optsrc = 1 + (it & 1))
#   plain    no certificate (kfok = 0): W = A^H g into the X buffer
#   cold     V is not the previous X (avok = 0) and N != 0: apply_A runs for its block
#   coldz    avok = 0 with N held as exact zero (nzero = 1, the N buffer holds garbage)
#   calm     in the form and CALM times as far from the fixed point as the others
#   done     stopped earlier
#   pass_    a convergence test pending on entry whose dual part passes
#   fail_b   ... fails, and mu is multiplied by rho;   fail_k  ... fails, mu stays
#   oy_this  opt_Y deferred in the buffer this launch overwrites;   oy_that  in the other one
# a calm realisation's distance from the fixed point relative to its neighbours': with the run cases' dynamics (the
# combined residual falls by 0.6 per iteration, the primal one by 0.2 in the first) and tol_rel = 1e-9 it passes neither
# test at it0 and the combined one at it0 + 1, so it stops one iteration into the run (test_unit_ref.py asserts it)
CALM = 3.7e-5
ROLES_MIX = ("enter", "form", "refused", "fused", "plain", "cold", "done", "form_d", "coldz")


def build(seed, m, n, b, kind, *, roles=("fused",), op="gyf", it=7, eps=1e-4, mu=2.0, bdev=0.1, **par):
    """The inputs of one launch, every realisation in the state its role names."""
    A, Z0, s2 = problem(seed, m, n, b, kind)
    rng = np.random.default_rng([s2, it, len(roles)])
    ops = operators(A)
    role = [roles[j % len(roles)] for j in range(b)]
    is_ = lambda *names: np.array([r in names for r in role])
    q = (it - 1) & 1
    yn_id = 2 - q
    calm = is_("calm")
    form = is_("form", "form_d", "calm")
    epsr, bdevr = np.where(calm, CALM * eps, eps)[:, None], np.where(calm, CALM * bdev, bdev)[:, None]
    Sold = np.where(form[:, None], 1e-3 * _cx(rng, b, m), 1e-3 * _cx(rng, b, m))
    Z = Z0 + np.where(form[:, None], Sold, 0) @ A.conj()           # the explicit iterate
    Nn = np.where(is_("cold")[:, None], 1e-2 * _cx(rng, b, n), 0)
    mus = mu * (1 + 0.25 * rng.random(b))
    V = Z - Nn / mus[:, None]
    AV = V @ A.T
    sc_ = np.abs(AV).mean() + 1e-30
    Y = AV + epsr * sc_ * _cx(rng, b, m)
    Yprev = Y + epsr * sc_ * _cx(rng, b, m)
    M = epsr * sc_ * _cx(rng, b, m)
    Bv = np.abs(AV) * (1 + bdevr * rng.random((b, m))) + 1e-3 * bdevr
    nz = np.linalg.norm(Z, axis=1)
    cold = is_("cold", "coldz")
    st = state_array(b, mu=mus, last_res=1e-2, opt_obj=1e3, kf0=nz, kf1=nz, kf2=nz, kf3=nz, kfcum=1e-7 * nz,
                     vbound=np.max(np.abs(np.ascontiguousarray(V).view(np.float64)), axis=1) * (1 + 2.0 ** -40),
                     fs0=np.sum(np.abs(Z) ** 2, axis=1), fs3=1e-8, obj2=4.0, nAX2=9.0, nY2=9.0, nJM2=1e-6, dY2=1e-6)
    fl = flags_array(b, iters=it - 1, nzero=~is_("cold"), avok=~cold, kfok=~is_("plain", "cold", "coldz"),
                     fzit=np.where(is_("fused", "fused_ox"), it - 2, it - 1), zit=it - 1, mzit=np.where(form, it - 1, 0),
                     msp=form, z0id=np.where(form, 1 if it & 1 else 2, 0), msp_pad=np.where(form, it - 3, 0),
                     done=is_("done"), optsrc=np.where(is_("form_d"), 4 + (it & 1), np.where(is_("fused_ox"), 1 + (it & 1), 0)),
                     optysrc=np.where(is_("form_d", "oy_this"), yn_id, np.where(is_("oy_that"), 3 - yn_id, 0)),
                     dpend=is_("pass_", "fail_b", "fail_k"))
    col = lambda k: STATE.index(k)
    st[is_("form_d", "oy_this", "oy_that", "fused_ox"), col("opt_obj")] = 1e-9               # nothing improves on it
    # room for one step (1e-4 ||Z|| at most here), not for 32 (8e-4 at least): 4e-4 ||Z|| below the bound's budget
    st[is_("refused"), col("kfcum")] = (1.0 - np.sqrt(0.95) - 4e-4) * nz[is_("refused")]
    pend = is_("pass_", "fail_b", "fail_k")
    st[pend, col("pd_nZ2")] = nz[pend] ** 2
    st[is_("fail_b", "fail_k"), col("pd_dZ2")] = 1.0
    st[is_("fail_b"), col("pd_rc")] = 1.0
    st[is_("fail_k", "pass_"), col("pd_rc")] = 1e-3
    inp = dict(PAR)
    inp.update(op=op, A=A, B=Bv, it=it, n=n, M=M, AX=np.where(cold[:, None], _cx(rng, b, m), AV), state=st, flags=fl,
               np=1, fl=(0.95,), optY=_cx(rng, b, m), optS=_cx(rng, b, m), optX=_cx(rng, b, n), Xcur=_cx(rng, b, n),
               X=_cx(rng, b, n), T=_cx(rng, b, m), g=1e-3 * _cx(rng, b, m), roles=role, **ops)
    inp[f"Y{q}"], inp[f"Y{1 - q}"] = Y, Yprev
    zc, zo, nc, no = ("Zb1", "Zb2", "Nb1", "Nb2") if it & 1 else ("Zb2", "Zb1", "Nb2", "Nb1")
    inp[zc], inp[zo] = np.where(form[:, None], Z0, Z), _cx(rng, b, n)
    inp[nc], inp[no] = np.where(is_("coldz")[:, None], _cx(rng, b, n), Nn), _cx(rng, b, n)
    inp[f"S{(it + 1) & 1}"], inp[f"S{it & 1}"] = Sold, 1e-3 * _cx(rng, b, m)
    inp[f"KY{q}"], inp[f"KY{1 - q}"] = Y @ ops["K"].T, _cx(rng, b, m)
    if op == "gyk" and not par.get("use_la", 1):
        inp["T"] = (Y - M / mus[:, None]) - AV            # the caller's T
    inp.update(par)
    return inp


def _cases():
    c = {}
    for name, (m, n, b, kind) in SHAPES.items():
        sd = 3 + m
        c[f"gyk-{name}"] = lambda a=(sd, m, n, b, kind): build(*a, op="gyk", roles=("fused", "cold", "done", "coldz"),
                                                              lazy=0, use_la=1, use_ax=1)
        c[f"gykT-{name}"] = lambda a=(sd, m, n, b, kind): build(*a, op="gyk", roles=("cold", "done"), lazy=0, use_la=0,
                                                               use_ax=0, yn_copy=1, it=8)
        c[f"gykL-{name}"] = lambda a=(sd, m, n, b, kind): build(
            *a, op="gyk", roles=("fused", "pass_", "cold", "fail_b", "oy_this", "fail_k", "oy_that", "done"), lazy=1,
            tol_rel=1e-2)
        c[f"gyf-{name}"] = lambda a=(sd, m, n, b, kind): build(*a, roles=("fused", "plain", "cold", "done", "coldz", "fused_ox"))
        c[f"gyfm-{name}"] = lambda a=(sd, m, n, b, kind): build(*a, roles=ROLES_MIX, msp=1, it=8)
        c[f"ahf-{name}"] = lambda a=(sd, m, n, b, kind): build(*a, op="ahf", roles=("fused", "plain", "done", "fused_ox"))
    mid = (11, 17, 33, 17, "pmj")
    big = (12, 121, 256, 35, "twin")
    for tag, a in (("m17", mid), ("m121", big)):
        pr = ("pass_", "fused", "fail_b", "fail_k")
        c[f"pend-stop-{tag}"] = lambda a=a: build(*a, roles=pr, tol_rel=1e-2)
        c[f"pend-fixed-{tag}"] = lambda a=a: build(*a, roles=pr, tol_rel=1e-2, fixed_iters=1)
        c[f"pend-plain-{tag}"] = lambda a=a: build(*a, op="gyk", roles=pr, tol_rel=1e-2, use_la=0, use_ax=1, lazy=1)
        c[f"defer-{tag}"] = lambda a=a: build(*a, roles=("oy_this", "oy_that", "form_d", "form"), msp=1)
        c[f"mixed-block-{tag}"] = lambda a=a: build(*a, roles=("fused",) * 5 + ("cold",) + ("fused",) * 13)
        c[f"entry-{tag}"] = lambda a=a: build(*a, roles=("enter", "refused"), msp=1)
        c[f"fail-it-{tag}"] = lambda a=a: build(*a, roles=("enter", "form", "fused"), msp=1, msp_fail_it=7)
        c[f"ctl0-{tag}"] = lambda a=a: build(*a, roles=("enter", "form", "fused"), msp=1, ctl=0)
        c[f"fixup-{tag}"] = lambda a=a: build(*a, roles=("enter", "form", "fused"), msp=1, maxiter=7)
        c[f"conv-{tag}"] = lambda a=a: build(*a, roles=("enter", "form"), msp=1, tol_rel=0.5)
        c[f"conv-fixed-{tag}"] = lambda a=a: build(*a, roles=("enter", "form"), msp=1, tol_rel=0.5, fixed_iters=1)
        c[f"rank1-{tag}"] = lambda a=a: dict(build(*a, roles=("enter", "refused", "form"), msp=1, np=2, fl=(0.5, 0.9999999)),
                                             rank_one=(np.arange(a[3]) % 2).astype(np.uint8))
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def ahead_case():
    """gyf_kernel's early return: block 0 of the batch is ahead (every live realisation has mzit >= it), block 1 runs."""
    inp = build(13, 17, 33, 35, "pmj", roles=("form", "done"), msp=1, it=8)
    fl = inp["flags"].copy()
    fl[:16, FLAGS.index("mzit")] = 9
    return dict(inp, flags=fl)


def zero_guard_case(m=17, n=33, b=17):
    """Y = M = AX = 0 (avok): T = 0, g = 0, AX + M/mu = 0: the zero guard, Y' = (B + mu) / (1 + mu) exactly."""
    inp = build(14, m, n, b, "pmj", op="gyk", roles=("fused",), lazy=1)
    z = np.zeros((b, m), complex)
    q = (inp["it"] - 1) & 1
    out = dict(inp, M=z, AX=z)
    out[f"Y{q}"] = z
    return out


RUN_VARIANTS = {
    "end": dict(tol_rel=1e-13, tol_abs=0.0),                      # stopped by it_end
    "failbound": dict(tol_rel=1e-13, tol_abs=0.0, fail_at=2),     # by a failed bound at it0 + 2: resume == it
    "pending": dict(tol_rel=1.2e-5, tol_abs=0.0),                 # by a test left pending: resume == it + 1
    "allstop": dict(),                                            # every realisation converges at it0
    "midstop": dict(tol_rel=1e-9, tol_abs=0.0),                   # one realisation converges at it0 + 1, the rest go on
    "fixed": dict(fixed_iters=1),                                 # converged under fixed_iters: flagged, goes on
    "notready": dict(tol_rel=1e-13, tol_abs=0.0),                 # the last block has a realisation outside the form
    "ahead": dict(tol_rel=1e-13, tol_abs=0.0),                    # block 0 is ahead: its mres stands
    "flush": dict(tol_rel=1e-13, tol_abs=0.0),                    # deferred opt_Y / opt_S on entry
    "done": dict(tol_rel=1e-13, tol_abs=0.0),                     # stopped realisations in every block
}


def run_case(name, variant="end", *, it0=9, it_end=14):
    """An m-space run's inputs: every realisation in the form through it0 - 1 (``variant`` breaks that)."""
    m, n, b, kind = RUN_SHAPES[name]
    par = dict(RUN_VARIANTS[variant])
    if "fail_at" in par:
        par["msp_fail_it"] = it0 + par.pop("fail_at")
    roles = {"flush": ("form_d", "form"), "done": ("form", "done", "form"),
             "midstop": ("form",) * 5 + ("calm",) + ("form",) * 13}.get(variant, ("form",))
    inp = build(21 + b, m, n, b, kind, roles=roles, msp=1, it=it0, bdev=2e-4, eps=1e-5, **par)
    inp.update(op="msr", it_end=it_end)
    fl = inp["flags"].copy()
    fi = FLAGS.index
    if variant == "notready":
        fl[b - 1, fi("msp")] = 0
    if variant == "ahead":
        fl[:16, fi("mzit")] = it0 + 2
        fl[:16, fi("mres")] = it0 + 3
    inp["flags"] = fl
    return inp
