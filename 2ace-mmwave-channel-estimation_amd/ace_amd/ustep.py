"""Host-side mirror of the test entry ``ace_unit_host`` (include/ace.h).

One launch of the unit path's fused iteration kernels (csrc/ace_i8gemm.hip) through the launcher a solve calls for
it: ``gyk`` (T, g = G T, the Y-step, K Y and the dual terms), ``gyf`` (the same body, the fused apply_AH pass, the
m-space entry and steps, the control in place), ``ahf`` (the fused apply_AH on its own), ``msr`` (an m-space run),
``ready`` (its readiness counts) and ``optx`` (opt_X of the best iterates kept in m-space form).  The state passes
through the host exactly, so launches are chained by handing a result's buffers, state, flags and counters back.
For tests (tests/test_gpu_unit.py); no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import LIB, check, UnitArgs, UNIT_VM, UNIT_VN

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_bp = C.POINTER(C.c_ubyte)

OPS = {"gyk": 0, "gyf": 1, "ahf": 2, "msr": 3, "ready": 4, "optx": 5}
STATE = ("mu", "last_res", "opt_obj", "nB", "vbound", "obj2", "nAX2", "nY2", "nJM2", "dY2", "dAtY", "nAtY", "kf0",
         "kf1", "kf2", "kf3", "kfcum", "pd_dZ2", "pd_nZ2", "pd_rc", "fs0", "fs3")
FLAGS = ("iters", "done", "status", "nzero", "avok", "optsrc", "optysrc", "kfok", "dpend", "fzit", "zit", "mzit", "msp",
         "z0id", "msp_pad", "mres")
VEC_M = UNIT_VM   # [batch][m] c128
VEC_N = UNIT_VN   # [batch][n] c128
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
class UnitResult:
    """What one launch left behind.  vec: every per-realisation buffer as it stands on the device after the launch
    ([batch][m] or [batch][n] c128; B: [batch][m] f64); ``guards`` maps each name to its trailing guard doubles;
    state / flags: [batch][len(STATE)] / [batch][len(FLAGS)]; K, G [m][m] c128 and c = (c, c^2) as the setup made
    them (None for ``ready``); resume, steps [4], vecw (msr); ready [3]; guard_ok: the control blocks' guard held."""
    vec: dict
    guards: dict
    state: np.ndarray
    flags: np.ndarray
    done_count: int
    mspcount: int
    K: np.ndarray
    G: np.ndarray
    c: np.ndarray
    resume: int
    steps: np.ndarray
    vecw: int
    ready: np.ndarray
    guard_ok: bool
    recert: np.ndarray = None   # [batch] int32 when the launch carried it (unit_host's recert), else None

    def __getattr__(self, k):
        if k in STATE:
            return self.state[:, STATE.index(k)]
        if k in FLAGS:
            return self.flags[:, FLAGS.index(k)]
        try:
            return self.__dict__["vec"][k]
        except KeyError:
            raise AttributeError(k) from None


def _ptr(x, tp=_dp):
    if x is None:
        return None
    return (x.view(np.float64) if x.dtype == np.complex128 else x).ctypes.data_as(tp)


def unit_host(op, *, batch, n, m, A=None, it=1, it_end=0, maxiter=1 << 30, q=None, fixed_iters=False, tol_rel=1e-4,
              tol_abs=1e-8, rho=1.05, lazy=True, use_la=True, use_ax=True, yn_copy=False, msp=False, ctl=True, np_=0,
              fl=(), room=32.0, rank_one=None, msp_fail_it=-1, waves=8, guard=None, sentinel=SENTINEL, done_count=0,
              mspcount=0, B=None, state=None, flags=None, recert=None, **vecs) -> UnitResult:
    """One launch (``ace_unit_host``).  vecs: any of VEC_M ([batch][m] complex) and VEC_N ([batch][n] complex).  q
    defaults to the solve's (it - 1) & 1; np_, fl: the rank profile's length and shares; guard defaults to 32 rows.
    recert ([batch] or a scalar; needs ``state``): the realisations' last fresh-reference request, carried as the
    trailing element of the state rows (``state_ext``); gyf may then raise a request, and the result has ``recert``."""
    if op not in OPS:
        raise ValueError(f"unknown op {op!r}")
    bad = set(vecs) - set(VEC_M) - set(VEC_N)
    if bad:
        raise TypeError(f"unknown ace_unit_args field(s) {sorted(bad)}")
    if len(fl) > 4:
        raise ValueError("at most 4 rank-profile shares")
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

    a = UnitArgs()
    a.op, a.batch, a.n, a.m, a.it, a.it_end, a.maxiter = OPS[op], int(batch), int(n), int(m), int(it), int(it_end), int(maxiter)
    a.q = (int(it) - 1) & 1 if q is None else int(q)
    a.fixed_iters, a.guard, a.done_count, a.mspcount = int(bool(fixed_iters)), guard, int(done_count), int(mspcount)
    a.lazy, a.use_la, a.use_ax, a.yn_copy = int(bool(lazy)), int(bool(use_la)), int(bool(use_ax)), int(bool(yn_copy))
    a.msp, a.ctl, a.np, a.msp_fail_it, a.waves = int(bool(msp)), int(bool(ctl)), int(np_), int(msp_fail_it), int(waves)
    a.tol_rel, a.tol_abs, a.rho, a.room, a.sentinel = float(tol_rel), float(tol_abs), float(rho), float(room), float(sentinel)
    for i, v in enumerate(fl):
        a.fl[i] = float(v)
    a.A = _ptr(arr(A, (m, n), "A"))
    a.B = _ptr(arr(B, (batch, m), "B", np.float64))
    for k in VEC_M:
        setattr(a, k, _ptr(arr(vecs.get(k), (batch, m), k)))
    for k in VEC_N:
        setattr(a, k, _ptr(arr(vecs.get(k), (batch, n), k)))
    ext = recert is not None
    if ext:
        if state is None:
            raise ValueError("recert travels with the state rows: pass state")
        rc = np.broadcast_to(np.asarray(recert, np.float64), (batch,))
        state = np.concatenate([np.asarray(state, np.float64).reshape(batch, len(STATE)), rc[:, None]], axis=1)
    a.state_ext = int(ext)
    a.state = _ptr(arr(state, (batch, len(STATE) + ext), "state", np.float64))
    a.flags = _ptr(arr(flags, (batch, len(FLAGS)), "flags", np.int32), _ip)
    a.rank_one = _ptr(arr(rank_one, (batch,), "rank_one", np.uint8), _bp)
    g = max(guard, 0)
    mz, nz, bz = max(m, 0), max(n, 0), max(batch, 0)
    raw = {k: np.empty(2 * bz * mz + g) for k in VEC_M}
    raw.update({k: np.empty(2 * bz * nz + g) for k in VEC_N})
    raw["B"] = np.empty(bz * mz + g)
    for k, x in raw.items():
        setattr(a, k + "_out", _ptr(x))
    K, G, c = np.zeros((mz, mz), np.complex128), np.zeros((mz, mz), np.complex128), np.zeros(2)
    a.K_out, a.G_out, a.c_out = _ptr(K), _ptr(G), _ptr(c)
    so, fo = np.zeros((bz, len(STATE) + ext)), np.zeros((bz, len(FLAGS)), np.int32)
    ints = {k: np.zeros(s, np.int32) for k, s in (("done_count_out", 1), ("mspcount_out", 1), ("resume", 1),
                                                  ("steps", 4), ("vecw", 1), ("ready", 3), ("guard_ok", 1))}
    a.state_out, a.flags_out = _ptr(so), _ptr(fo, _ip)
    for k, x in ints.items():
        setattr(a, k, _ptr(x, _ip))
    check(LIB.ace_unit_host(C.byref(a)))
    vec, guards = {}, {}
    for k, x in raw.items():
        body = x[:x.size - g]
        guards[k] = x[x.size - g:].copy()
        vec[k] = body.copy().reshape(batch, m) if k == "B" else body.copy().view(np.complex128).reshape(batch, -1)
    have = op != "ready"
    rc_out = so[:, len(STATE)].astype(np.int32) if ext else None
    so = np.ascontiguousarray(so[:, :len(STATE)])
    return UnitResult(vec=vec, guards=guards, state=so, flags=fo, recert=rc_out, done_count=int(ints["done_count_out"][0]),
                      mspcount=int(ints["mspcount_out"][0]), K=K if have else None, G=G if have else None,
                      c=c if have else None, resume=int(ints["resume"][0]), steps=ints["steps"],
                      vecw=int(ints["vecw"][0]), ready=ints["ready"], guard_ok=bool(ints["guard_ok"][0]))
