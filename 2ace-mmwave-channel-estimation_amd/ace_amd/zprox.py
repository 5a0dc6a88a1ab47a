"""Host-side mirror of the Z-step test entry ``ace_zprox_host`` (include/ace.h).

One Z-step of the ADMM iteration -- ``Z' = ArgMinZ(X + N/mu)``, ``N' = N + mu (X - Z')`` and the iteration control
(inferLowRankV4_multi.m:423-485, :344-381) -- through the launcher call a solve makes for it: the one-wave kernel
at r = 1 (Jacobi, the tridiagonal top-K path, the rank-one Lanczos path, the Ky Fan certificate, the wmode /
ping-pong form, the lean kernel), the four-wave kernel at r > 1.  For tests (tests/test_gpu_zprox.py); no CPU
fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import LIB, check, ACE_VARIANT_A2ONLY, ACE_VARIANT_NUCLEAR

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_bp = C.POINTER(C.c_ubyte)

STATE_IN = ("mu", "last_res", "opt_obj", "obj2", "nAX2", "nY2", "nJM2", "dY2", "dAtY", "nAtY", "kfcum")   # then kf[4]
FLAGS_IN = ("done", "nzero", "kfok", "optsrc")
NIN, NFLAG, NOUT, NFLAGOUT = 15, 4, 9, 8


class ZproxArgs(C.Structure):
    """Mirror of ``ace_zprox_args`` (include/ace.h)."""
    _fields_ = [("variant", C.c_int), ("batch", C.c_int), ("tx", C.c_int), ("rx", C.c_int), ("r", C.c_int),
                ("m", C.c_int), ("np", C.c_int), ("rl", C.c_int * 4), ("fl", C.c_double * 4),
                ("init", C.c_int), ("row_mode", C.c_int), ("it", C.c_int), ("fixed_iters", C.c_int),
                ("warm", C.c_int), ("tkeig", C.c_int), ("r1lz", C.c_int), ("zcert", C.c_int), ("wmode", C.c_int),
                ("pingpong", C.c_int), ("lean", C.c_int), ("reserved", C.c_int),
                ("tol_rel", C.c_double), ("tol_abs", C.c_double), ("rho", C.c_double), ("sentinel", C.c_double),
                ("rank_one", _bp), ("X", _dp), ("Z", _dp), ("N", _dp), ("Q", _dp), ("state", _dp), ("flags", _ip),
                ("Zo", _dp), ("No", _dp), ("Qo", _dp), ("optX", _dp), ("Xcur", _dp), ("state_out", _dp),
                ("flags_out", _ip), ("tkcnt", _ip)]


LIB.ace_zprox_host.argtypes = [C.POINTER(ZproxArgs)]
LIB.ace_zprox_host.restype = C.c_int

SENTINEL = -7.25e77   # default fill of the output buffers (both components)


@dataclass
class ZproxResult:
    """What one Z-step left behind.  Z, N: [batch][r][n] (in place: the buffers after the step; ping-pong: the
    output pair, untouched entries ``sentinel (1 + 1j)``); Q [batch][tx][tx]; optX, Xcur [batch][nc][n]; the
    per-realisation arrays are [batch] (kf: [batch][4]); tkcnt: top-K tridiagonal uses, Jacobi fallbacks."""
    Z: np.ndarray
    N: np.ndarray
    Q: np.ndarray
    optX: np.ndarray
    Xcur: np.ndarray
    mu: np.ndarray
    last_res: np.ndarray
    opt_obj: np.ndarray
    vbound: np.ndarray
    kf: np.ndarray
    kfcum: np.ndarray
    iters: np.ndarray
    done: np.ndarray
    status: np.ndarray
    nzero: np.ndarray
    avok: np.ndarray
    kfok: np.ndarray
    optsrc: np.ndarray
    zit: np.ndarray
    tkcnt: np.ndarray


def _c(x, shape, name):
    if x is None:
        return None
    x = np.ascontiguousarray(np.asarray(x, dtype=np.complex128))
    if x.shape != shape:
        raise ValueError(f"{name}: expected shape {shape}, got {x.shape}")
    return x


def _ptr(x, tp=_dp):
    if x is None:
        return None
    return (x.view(np.float64) if x.dtype == np.complex128 else x).ctypes.data_as(tp)


def zprox_host(X, tx, rx, *, variant="A2only", r=1, m=None, profile=None, rank_one=None, init=False, Z=None, N=None,
               Q=None, mu=1.0, last_res=0.0, opt_obj=0.0, obj2=0.0, nAX2=0.0, nY2=0.0, nJM2=0.0, dY2=0.0, dAtY=0.0,
               nAtY=0.0, kf=None, kfcum=0.0, done=0, nzero=0, kfok=0, optsrc=0, tol_rel=1e-3, tol_abs=1e-4, rho=1.05,
               it=1, fixed_iters=True, row_mode=True, warm=False, tkeig=0, r1lz=False, zcert=False, wmode=False,
               pingpong=False, lean=False, sentinel=SENTINEL) -> ZproxResult:
    """One Z-step (``ace_zprox_host``).

    X: [batch][r][n] (or [batch][n] at r = 1), n = tx rx, each column a column-major tx x rx matrix; in wmode it holds
    W = A^H g.  profile: (rl, fl) or None for ``rank_profile(tx, rx, m, n, 0)`` (m defaults to n).  The control
    block inputs (mu ... optsrc) are per realisation; scalars broadcast.
    """
    X = np.asarray(X, dtype=np.complex128)
    n = tx * rx
    if X.ndim == 2 and r == 1:
        X = X[:, None, :]
    batch = X.shape[0]
    shape = (batch, r, n)
    X, Z, N = _c(X, shape, "X"), _c(Z, shape, "Z"), _c(N, shape, "N")
    Q = _c(Q, (batch, tx, tx), "Q")
    nc = r if (r == 1 or row_mode) else 1
    a = ZproxArgs()
    a.variant = {"A2only": ACE_VARIANT_A2ONLY, "A2nuclear": ACE_VARIANT_NUCLEAR}[variant]
    a.batch, a.tx, a.rx, a.r, a.m = batch, int(tx), int(rx), int(r), int(n if m is None else m)
    if profile is not None:
        rl, fl = profile
        a.np = len(rl)
        for p, (rr, ff) in enumerate(zip(rl, fl)):
            a.rl[p], a.fl[p] = int(rr), float(ff)
    a.init, a.row_mode, a.it, a.fixed_iters = int(bool(init)), int(bool(row_mode)), int(it), int(bool(fixed_iters))
    a.warm, a.tkeig, a.r1lz, a.zcert = int(bool(warm)), int(tkeig), int(bool(r1lz)), int(bool(zcert))
    a.wmode, a.pingpong, a.lean = int(bool(wmode)), int(bool(pingpong)), int(bool(lean))
    a.tol_rel, a.tol_abs, a.rho, a.sentinel = float(tol_rel), float(tol_abs), float(rho), float(sentinel)

    def per(v, dt=np.float64):
        return np.broadcast_to(np.asarray(v, dt), (batch,))

    state = np.zeros((batch, NIN))
    for k, v in enumerate((mu, last_res, opt_obj, obj2, nAX2, nY2, nJM2, dY2, dAtY, nAtY, kfcum)):
        state[:, k] = per(v)
    if kf is not None:
        state[:, 11:15] = np.broadcast_to(np.asarray(kf, np.float64), (batch, 4))
    flags = np.zeros((batch, NFLAG), np.int32)
    for k, v in enumerate((done, nzero, kfok, optsrc)):
        flags[:, k] = per(v, np.int32)
    r1 = None if rank_one is None else np.ascontiguousarray(per(rank_one, np.uint8))
    Zo, No = np.empty(shape, np.complex128), np.empty(shape, np.complex128)
    Qo = np.empty((batch, tx, tx), np.complex128)
    optX, Xcur = np.empty((batch, nc, n), np.complex128), np.empty((batch, nc, n), np.complex128)
    so, fo = np.zeros((batch, NOUT)), np.zeros((batch, NFLAGOUT), np.int32)
    tk = np.zeros(2, np.int32)
    a.rank_one = _ptr(r1, _bp)
    a.X, a.Z, a.N, a.Q, a.state, a.flags = _ptr(X), _ptr(Z), _ptr(N), _ptr(Q), _ptr(state), _ptr(flags, _ip)
    a.Zo, a.No, a.Qo, a.optX, a.Xcur = _ptr(Zo), _ptr(No), _ptr(Qo), _ptr(optX), _ptr(Xcur)
    a.state_out, a.flags_out, a.tkcnt = _ptr(so), _ptr(fo, _ip), _ptr(tk, _ip)
    check(LIB.ace_zprox_host(C.byref(a)))
    return ZproxResult(Z=Zo, N=No, Q=Qo, optX=optX, Xcur=Xcur, mu=so[:, 0].copy(), last_res=so[:, 1].copy(),
                       opt_obj=so[:, 2].copy(), vbound=so[:, 3].copy(), kf=so[:, 4:8].copy(), kfcum=so[:, 8].copy(),
                       iters=fo[:, 0].copy(), done=fo[:, 1].copy(), status=fo[:, 2].copy(), nzero=fo[:, 3].copy(),
                       avok=fo[:, 4].copy(), kfok=fo[:, 5].copy(), optsrc=fo[:, 6].copy(), zit=fo[:, 7].copy(),
                       tkcnt=tk)
