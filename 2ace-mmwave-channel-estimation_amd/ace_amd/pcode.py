"""Host-side mirror of the test entry ``ace_pc_host`` (include/ace.h).

One operation of the private code-image kernels (csrc/ace_private.hip) through the launcher a solve calls for it:
``pack`` (the 2-bit code images), ``kmat`` (I + K), ``inv`` (the Schur recursion or the blocked Gauss-Jordan on a
caller's matrices), ``tiles``, ``apply_a`` (P0 = A X0) and ``step`` (one ``pgk_kernel`` launch).  The state passes
through the host exactly, so two launches are chained by handing a result back with ``PcResult.next()``.
For tests (tests/test_gpu_pc.py); no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import LIB, check, PcArgs

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint32)

OPS = {"pack": 0, "kmat": 1, "inv": 2, "tiles": 3, "apply_a": 4, "step": 5}
FORMS = {"schur": 0, "gj": 1}
STATE = ("mu", "opt_obj", "vbound", "obj2", "nAX2", "nY2", "nJM2", "dY2", "dAtY", "nAtY")
FLAGS = ("done", "avok", "nzero", "optysrc")
VEC_M = ("Yo", "M", "AX", "Yn", "optY")   # [batch][m] c128 inputs of a step (B: [batch][m] f64)
VEC_N = ("Z", "N")                         # [batch][n] c128
SENTINEL = -7.25e77   # default fill of the buffers the caller does not supply, and of every guard


def dims(m, n):
    """The sizes of ``pc_dims`` (csrc/ace_private.hip) that shape this entry's arrays."""
    mt, nct = (m + 15) // 16, (n + 15) // 16
    nkgH, nkgA = (mt + 7) // 8, (nct + 7) // 8
    return dict(mt=mt, mp=16 * mt, mp32=32 * ((m + 31) // 32), nb32=(m + 31) // 32, ntile=mt * (mt + 1) // 2, nct=nct,
                nkgH=nkgH, nkgA=nkgA, nwR=nct, nH=nct * nkgH * 128, nA=mt * nkgA * 128, nR=m * nct)


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
class PcResult:
    """What one operation left behind, as the device buffers stand after the launch.  ``vec``: Yo, M, AX, Yn, optY, P0
    [batch][m] c128, B [batch][m] f64, W, Z, N [batch][n] c128, cb [batch], Gw [batch][mp32][mp32] c128, Gt
    [batch][ntile][16][16] c128 (column-major tiles), cH / cA / cR the three dword images [batch][...]; ``guards``
    maps a buffer's name to its trailing guard (``codes``: the dwords after the three images); flag: pc_pack's;
    state / flags: [batch][len(STATE)] / [batch][len(FLAGS)]; guard_ok: the control blocks' guard held."""
    vec: dict
    guards: dict
    state: np.ndarray
    flags: np.ndarray
    flag: int
    guard_ok: bool
    sentinel: float

    def __getattr__(self, k):
        if k in STATE:
            return self.state[:, STATE.index(k)]
        if k in FLAGS:
            return self.flags[:, FLAGS.index(k)]
        try:
            return self.__dict__["vec"][k]
        except KeyError:
            raise AttributeError(k) from None

    def guards_hold(self, names=None):
        """Every guard (or the named ones) still holds the sentinel (the code images': 0xFF bytes)."""
        for k, gd in self.guards.items():
            if names is not None and k not in names:
                continue
            want = np.uint32(0xFFFFFFFF) if gd.dtype == np.uint32 else self.sentinel
            if not (gd == want).all():
                return False
        return True

    def next(self):
        """The inputs of the following step: the Y ping-pong pair swapped, the rest handed back."""
        v = self.vec
        return dict(Yo=v["Yn"], Yn=v["Yo"], M=v["M"], AX=v["AX"], optY=v["optY"], B=v["B"], Z=v["Z"], N=v["N"],
                    state=self.state, flags=self.flags)


def _ptr(x, tp=_dp):
    if x is None:
        return None
    return (x.view(np.float64) if x.dtype == np.complex128 else x).ctypes.data_as(tp)


def pc_host(op, *, batch, m, n=16, form="schur", yn_id=0, guard=None, sentinel=SENTINEL, A=None, Gin=None, X0=None,
            G=None, B=None, state=None, flags=None, **vecs) -> PcResult:
    """One operation (``ace_pc_host``).  vecs: any of VEC_M ([batch][m] complex) and VEC_N ([batch][n] complex).
    guard defaults to 64 doubles / dwords."""
    if op not in OPS:
        raise ValueError(f"unknown op {op!r}")
    if form not in FORMS:
        raise ValueError(f"unknown form {form!r}")
    bad = set(vecs) - set(VEC_M) - set(VEC_N)
    if bad:
        raise TypeError(f"unknown ace_pc_args field(s) {sorted(bad)}")
    guard = 64 if guard is None else int(guard)
    d = dims(max(m, 1), max(n, 1))
    keep = []

    def arr(x, shape, name, dt=np.complex128):
        if x is None:
            return None
        x = np.ascontiguousarray(np.asarray(x, dtype=dt))
        if x.shape != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {x.shape}")
        keep.append(x)
        return x

    a = PcArgs()
    a.op, a.form, a.batch, a.m, a.n = OPS[op], FORMS[form], int(batch), int(m), int(n)
    a.yn_id, a.guard = int(yn_id), guard
    a.sentinel = float(sentinel)
    a.A = _ptr(arr(A, (batch, m, n), "A"))
    a.Gin = _ptr(arr(Gin, (batch, d["mp32"], d["mp32"]), "Gin"))
    a.X0 = _ptr(arr(X0, (batch, n), "X0"))
    a.G = _ptr(arr(G, (batch, m, m), "G"))
    a.B = _ptr(arr(B, (batch, m), "B", np.float64))
    for k in VEC_M:
        setattr(a, k, _ptr(arr(vecs.get(k), (batch, m), k)))
    for k in VEC_N:
        setattr(a, k, _ptr(arr(vecs.get(k), (batch, n), k)))
    a.state = _ptr(arr(state, (batch, len(STATE)), "state", np.float64))
    a.flags = _ptr(arr(flags, (batch, len(FLAGS)), "flags", np.int32), _ip)
    g, bq, mq, nq = max(guard, 0), max(batch, 0), max(m, 0), max(n, 0)
    ncode = bq * (d["nH"] + d["nA"] + d["nR"])
    sizes = dict(cb=bq, Gw=2 * bq * d["mp32"] ** 2, Gt=bq * d["ntile"] * 512, P0=2 * bq * mq, B=bq * mq, W=2 * bq * nq,
                 Z=2 * bq * nq, N=2 * bq * nq)
    sizes.update({k: 2 * bq * mq for k in VEC_M})
    raw = {k: np.empty(s + g) for k, s in sizes.items()}
    codes = np.empty(ncode + g, np.uint32)
    for k in raw:
        setattr(a, k if k in ("cb", "Gw", "Gt", "P0", "W") else k + "_out", _ptr(raw[k]))
    a.codes = _ptr(codes, _up)
    so, fo = np.zeros((bq, len(STATE))), np.zeros((bq, len(FLAGS)), np.int32)
    fl, gok = np.zeros(1, np.int32), np.zeros(1, np.int32)
    a.state_out, a.flags_out, a.flag_out, a.guard_ok = _ptr(so), _ptr(fo, _ip), _ptr(fl, _ip), _ptr(gok, _ip)
    check(LIB.ace_pc_host(C.byref(a)))
    vec, guards = {}, {}
    for k, x in raw.items():
        body = x[:x.size - g].copy()
        guards[k] = x[x.size - g:].copy()
        if k == "cb":
            vec[k] = body
        elif k == "B":
            vec[k] = body.reshape(batch, m)
        elif k == "Gw":
            vec[k] = body.view(np.complex128).reshape(batch, d["mp32"], d["mp32"])
        elif k == "Gt":
            vec[k] = body.view(np.complex128).reshape(batch, d["ntile"], 16, 16)
        else:
            vec[k] = body.view(np.complex128).reshape(batch, -1)
    o1, o2 = batch * d["nH"], batch * (d["nH"] + d["nA"])
    vec["cH"] = codes[:o1].copy().reshape(batch, d["nH"])
    vec["cA"] = codes[o1:o2].copy().reshape(batch, d["nA"])
    vec["cR"] = codes[o2:ncode].copy().reshape(batch, d["nR"])
    guards["codes"] = codes[ncode:].copy()
    return PcResult(vec=vec, guards=guards, state=so, flags=fo, flag=int(fl[0]), guard_ok=bool(gok[0]),
                    sentinel=float(sentinel))
