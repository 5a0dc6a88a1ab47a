"""Host-side mirror of the test entry ``ace_nms_host`` (include/ace.h).

One operation of the A2nuclear m-space iteration (csrc/ace_nucmsp.hip) through the launcher a solve calls for it:
``init`` (E_prev = X_init), ``step`` (the dense G and K packed in fragment order, then one iteration), ``fin`` (only
the convergence tests left pending) and ``out`` (the parts of the selected iterate).  The state passes through the
host exactly, so ``init -> step -> ... -> fin -> out`` is chained by handing a result back with ``NmsResult.next()``.
For tests (tests/test_gpu_nms.py); no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import LIB, check, NmsArgs

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)

OPS = {"init": 0, "step": 1, "fin": 2, "out": 3}
STATE = ("mu", "last_res", "opt_obj", "na", "naz", "nbeta", "nep2", "nopt_a", "ncur_a", "pd_dZ2", "pd_nZ2", "pd_rc",
         "obj2", "nAX2", "nY2", "nJM2", "dY2", "dAtY", "nAtY", "nx0")
FLAGS = ("iters", "done", "status", "dpend")
VEC_IN = ("Yo", "Yn", "M", "Eo", "AEo", "optW", "optY", "curW")          # [batch][m] c128 inputs
VEC_OUT = ("Yo", "Yn", "M", "Eo", "En", "AEo", "AEn", "optW", "optY", "curW", "Wsel")
SENTINEL = -7.25e77   # default fill of the buffers the caller does not supply, and of every guard


def state_array(batch, **kw):
    """[batch][len(STATE)] with mu = 1 and the named columns set (scalars broadcast)."""
    s = np.zeros((batch, len(STATE)))
    s[:, 0] = 1.0
    for k, v in kw.items():
        s[:, STATE.index(k)] = v
    return s


def flags_array(batch, **kw):
    f = np.zeros((batch, len(FLAGS)), np.int32)
    for k, v in kw.items():
        f[:, FLAGS.index(k)] = v
    return f


@dataclass
class NmsResult:
    """What one operation left behind.  Vector arrays are [batch][m] c128 (V: [batch][n], B: [batch][m] f64) as the
    device buffers stand after the launch; ``guards`` maps each name to its trailing guard doubles; state / flags:
    [batch][len(STATE)] / [batch][len(FLAGS)]; done_count: int; guard_ok: the control blocks' guard held."""
    vec: dict
    guards: dict
    state: np.ndarray
    flags: np.ndarray
    done_count: int
    guard_ok: bool

    def __getattr__(self, k):
        if k in STATE:
            return self.state[:, STATE.index(k)]
        if k in FLAGS:
            return self.flags[:, FLAGS.index(k)]
        try:
            return self.__dict__["vec"][k]
        except KeyError:
            raise AttributeError(k) from None

    def next(self):
        """The inputs of the following step / fin: the ping-pong pairs swapped, the rest handed back."""
        v = self.vec
        return dict(Yo=v["Yn"], Yn=v["Yo"], M=v["M"], Eo=v["En"], AEo=v["AEn"], optW=v["optW"], optY=v["optY"],
                    curW=v["curW"], state=self.state, flags=self.flags, done_count=self.done_count)


def _ptr(x, tp=_dp):
    if x is None:
        return None
    return (x.view(np.float64) if x.dtype == np.complex128 else x).ctypes.data_as(tp)


def nms_host(op, *, batch, n, m, it=1, fixed_iters=False, tol_rel=1e-4, tol_abs=1e-8, rho=1.05, guard=None,
             sentinel=SENTINEL, done_count=0, Xinit=None, P0=None, G=None, K=None, B=None, state=None, flags=None,
             **vecs) -> NmsResult:
    """One operation (``ace_nms_host``).  vecs: any of VEC_IN, [batch][m] complex.  guard defaults to 32 rows."""
    if op not in OPS:
        raise ValueError(f"unknown op {op!r}")
    bad = set(vecs) - set(VEC_IN)
    if bad:
        raise TypeError(f"unknown ace_nms_args field(s) {sorted(bad)}")
    guard = 2 * 32 * max(m, n, 1) if guard is None else int(guard)
    keep = []

    def arr(x, shape, name, dt=np.complex128):
        if x is None:
            return None
        x = np.ascontiguousarray(np.asarray(x, dtype=dt))
        if x.shape != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {x.shape}")
        keep.append(x)
        return x

    a = NmsArgs()
    a.op, a.batch, a.n, a.m, a.it = OPS[op], int(batch), int(n), int(m), int(it)
    a.fixed_iters, a.guard, a.done_count = int(bool(fixed_iters)), guard, int(done_count)
    a.tol_rel, a.tol_abs, a.rho, a.sentinel = float(tol_rel), float(tol_abs), float(rho), float(sentinel)
    a.Xinit = _ptr(arr(Xinit, (batch, n), "Xinit"))
    a.P0 = _ptr(arr(P0, (batch, m), "P0"))
    a.G, a.K = _ptr(arr(G, (m, m), "G")), _ptr(arr(K, (m, m), "K"))
    a.B = _ptr(arr(B, (batch, m), "B", np.float64))
    for k in VEC_IN:
        setattr(a, k, _ptr(arr(vecs.get(k), (batch, m), k)))
    a.state = _ptr(arr(state, (batch, len(STATE)), "state", np.float64))
    a.flags = _ptr(arr(flags, (batch, len(FLAGS)), "flags", np.int32), _ip)
    g = max(guard, 0)
    raw = {k: np.empty(2 * batch * max(m, 0) + g) for k in VEC_OUT}
    raw["B"] = np.empty(batch * max(m, 0) + g)
    raw["V"] = np.empty(2 * batch * max(n, 0) + g)
    for k in VEC_OUT + ("B",):
        setattr(a, k if k in ("Wsel",) else k + "_out", _ptr(raw[k]))
    a.V = _ptr(raw["V"])
    so, fo = np.zeros((batch, len(STATE))), np.zeros((batch, len(FLAGS)), np.int32)
    dc, gok = np.zeros(1, np.int32), np.zeros(1, np.int32)
    a.state_out, a.flags_out, a.done_count_out, a.guard_ok = _ptr(so), _ptr(fo, _ip), _ptr(dc, _ip), _ptr(gok, _ip)
    check(LIB.ace_nms_host(C.byref(a)))
    vec, guards = {}, {}
    for k, x in raw.items():
        body = x[:x.size - g]
        guards[k] = x[x.size - g:].copy()
        vec[k] = body.copy().reshape(batch, m) if k == "B" else body.copy().view(np.complex128).reshape(batch, -1)
    return NmsResult(vec=vec, guards=guards, state=so, flags=fo, done_count=int(dc[0]), guard_ok=bool(gok[0]))
