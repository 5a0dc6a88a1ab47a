"""Host-side mirror of the test entry ``ace_pl_host`` (include/ace.h).

One operation of the PhaseLift step kernels (csrc/ace_phaselift.hip) through the launcher the solve calls for it: the
steps of the TFOCS Auslender-Teboulle iteration (``theta`` ... ``iterate``), its GEMMs (``gy``, ``zasm``,
``apply_a``), the setup (``chol``, ``transpose``) and the output (``final_vec``, ``outputs``).  Arrays and state pass
through the host exactly, so launches are chained by handing a result's arrays back.
For tests (tests/test_gpu_pl.py); no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import LIB, check, PlArgs, PL_F64, PL_I32

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)

OPS = {k: i for i, k in enumerate((
    "init", "outer_begin", "theta", "make_y", "set_ay", "grad", "gy", "prox_in", "assemble", "zasm", "take_z", "apply_a",
    "make_x", "set_ax", "backtrack", "iterate", "chol", "transpose", "final_vec", "outputs"))}
STATE = ("L", "L_old", "theta", "theta_old", "f_x", "f_y", "C_x", "C_z", "cntr_Ax", "cntr_Ay", "xy_sq", "nx2", "ndx2",
         "dot_xy_g", "localL", "step", "n_iter", "restart_iter", "backtrack_simple", "backtrack_steps", "have_gAy",
         "have_gy", "have_gAx", "ycomp", "need_Ay", "need_Ax", "inner", "done", "status")
NFLOAT = 16              # the leading f64 fields of STATE; the rest are int32 carried as exact doubles
SENTINEL = -7.25e77      # default fill of the buffers the caller does not supply, and of every guard
ISENTINEL = 0x5A5A5A5A   # the same for the int32 buffers
MATS = ("x", "xo", "z", "zo", "y", "G", "Znew", "P", "VT", "V", "C")            # [batch][d][d] c128
VECS = ("Ax", "Axo", "Az", "Azo", "Ay", "gAy", "gAx", "Aex", "bvec")              # [batch][m] f64
PARAMS = dict(cntr_reset=50, restart=200, maxIts=4000, alpha=0.9, beta=0.5, Lexact=np.inf, tol=1e-10, L0=1.0)
PARAMS["lambda"] = 5e-2


def shapes(batch, m, d):
    """name -> (shape, dtype) of every array of the entry."""
    s = {k: ((batch, d, d), np.complex128) for k in MATS}
    s.update({k: ((batch, m), np.float64) for k in VECS})
    s.update(R=((d, m), np.complex128), RT=((m, d), np.complex128), Pg=((batch, d, m), np.complex128),
             T=((batch, d, m), np.complex128), tau=((batch,), np.float64), lam=((batch, d), np.float64),
             misc=((batch, 3), np.float64), K=((m, m), np.complex128), cholR=((m, m), np.complex128),
             V1=((batch, d), np.complex128), w=((batch, d), np.complex128), act=((batch,), np.int32),
             cnt=((9,), np.int32), ok=((1,), np.int32), iters=((batch,), np.int32), status=((batch,), np.int32))
    return s


def state_array(batch, **kw):
    """[batch][len(STATE)] zeros with the named columns set (scalars broadcast)."""
    s = np.zeros((batch, len(STATE)))
    for k, v in kw.items():
        s[:, STATE.index(k)] = v
    return s


@dataclass
class PlResult:
    """What one operation left behind, as the device buffers stand after the launch: ``arr`` maps every array's name
    to its contents, ``guards`` to its trailing guard; state: [batch][len(STATE)]; guard_ok: the entry's own
    comparison of every guard and every buffer the operation must not write."""
    arr: dict
    guards: dict
    state: np.ndarray
    guard_ok: bool
    sentinel: float

    def __getattr__(self, k):
        if k in STATE:
            return self.state[:, STATE.index(k)]
        try:
            return self.__dict__["arr"][k]
        except KeyError:
            raise AttributeError(k) from None

    def guards_hold(self):
        for k, gd in self.guards.items():
            want = np.int32(ISENTINEL) if gd.dtype == np.int32 else self.sentinel
            if not (gd == want).all():
                return False
        return True


def _ptr(x, tp=_dp):
    if x is None:
        return None
    return (x.view(np.float64) if x.dtype == np.complex128 else x).ctypes.data_as(tp)


def pl_host(op, *, batch, m, d, reduced=0, guard=None, sentinel=SENTINEL, state=None, **kw) -> PlResult:
    """One operation (``ace_pl_host``).  kw: the scalars of PARAMS (``lam_reg`` for lambda) and any array of ``shapes``.
    guard defaults to 64 doubles / ints."""
    if op not in OPS:
        raise ValueError(f"unknown op {op!r}")
    par = dict(PARAMS)
    if "lam_reg" in kw:
        par["lambda"] = kw.pop("lam_reg")
    for k in list(kw):
        if k in par:
            par[k] = kw.pop(k)
    sh = shapes(max(batch, 0), max(m, 0), max(d, 0))
    bad = set(kw) - set(sh)
    if bad:
        raise TypeError(f"unknown ace_pl_args field(s) {sorted(bad)}")
    guard = 64 if guard is None else int(guard)
    keep = []

    def arr(x, shape, name, dt):
        if x is None:
            return None
        x = np.ascontiguousarray(np.asarray(x, dtype=dt))
        if x.shape != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {x.shape}")
        keep.append(x)
        return x

    a = PlArgs()
    a.op, a.batch, a.m, a.d, a.guard, a.reduced = OPS[op], int(batch), int(m), int(d), guard, int(reduced)
    for k, v in par.items():
        setattr(a, k, float(v) if k in ("lambda", "alpha", "beta", "Lexact", "tol", "L0") else int(v))
    a.sentinel = float(sentinel)
    for k in PL_F64 + PL_I32:
        shape, dt = sh[k]
        setattr(a, k, _ptr(arr(kw.get(k), shape, k, dt), _ip if dt == np.int32 else _dp))
    a.state = _ptr(arr(state, (batch, len(STATE)), "state", np.float64))
    g = max(guard, 0)
    raw = {}
    for k in PL_F64 + PL_I32:
        shape, dt = sh[k]
        n = int(np.prod(shape)) * (2 if dt == np.complex128 else 1)
        raw[k] = np.empty(n + g, np.int32 if dt == np.int32 else np.float64)
        setattr(a, k + "_out", _ptr(raw[k], _ip if dt == np.int32 else _dp))
    so, gok = np.zeros((max(batch, 0), len(STATE))), np.zeros(1, np.int32)
    a.state_out, a.guard_ok = _ptr(so), _ptr(gok, _ip)
    check(LIB.ace_pl_host(C.byref(a)))
    out, guards = {}, {}
    for k, x in raw.items():
        shape, dt = sh[k]
        body = x[:x.size - g].copy()
        guards[k] = x[x.size - g:].copy()
        out[k] = (body.view(np.complex128) if dt == np.complex128 else body).reshape(shape)
    return PlResult(arr=out, guards=guards, state=so, guard_ok=bool(gok[0]), sentinel=float(sentinel))
