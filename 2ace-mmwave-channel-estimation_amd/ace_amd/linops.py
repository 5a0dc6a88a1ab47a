"""Host-side mirror of the operator test entries ``ace_linop_host`` / ``ace_zgemm_host`` (include/ace.h).

One application of a linear operator of the ADMM iteration -- ``T = (Y - M/mu) - A (Z - N/mu)``,
``X = (Z - N/mu) + A^H g``, ``K Y``, ``G T`` -- through the launcher calls a solve makes for it, on the f64
matrix-core GEMM / GEMV path or the exact int8 digit planes.  For tests (tests/test_gpu_linops.py); no CPU
fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import LIB, check

OPS = {"A": 0, "AH": 1, "K": 2, "G": 3, "setup": 4}
PATHS = {"f64": 0, "f64_fused": 1, "i8": 2}

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class LinopArgs(C.Structure):
    """Mirror of ``ace_linop_args`` (include/ace.h)."""
    _fields_ = [("op", C.c_int), ("path", C.c_int), ("a_shared", C.c_int), ("batch", C.c_int), ("m", C.c_int),
                ("n", C.c_int), ("rcols", C.c_int), ("reserved", C.c_int),
                ("A", _dp), ("Z", _dp), ("N", _dp), ("Y", _dp), ("M", _dp), ("g", _dp), ("AX", _dp),
                ("mu", _dp), ("vbound", _dp), ("done", _ip), ("nzero", _ip), ("avok", _ip),
                ("sentinel", C.c_double), ("out", _dp), ("out2", _dp), ("out3", _dp)]


LIB.ace_linop_host.argtypes = [C.POINTER(LinopArgs)]
LIB.ace_linop_host.restype = C.c_int
LIB.ace_zgemm_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_longlong, C.c_int, C.c_longlong,
                               _dp, C.c_longlong, C.c_int, C.c_longlong, _dp, _dp, C.c_longlong, C.c_int,
                               C.c_longlong, C.c_int, _dp, C.c_longlong, C.c_longlong]
LIB.ace_zgemm_host.restype = C.c_int

SENTINEL = -7.25e77   # default fill of the output rows (both components)


def _c(x, shape):
    if x is None:
        return None
    x = np.ascontiguousarray(np.asarray(x, dtype=np.complex128))
    if x.shape != shape:
        raise ValueError(f"expected shape {shape}, got {x.shape}")
    return x


def _ptr(x, tp=_dp):
    if x is None:
        return None
    return (x.view(np.float64) if x.dtype == np.complex128 else x).ctypes.data_as(tp)


def linop_host(op, path, A, *, Z=None, N=None, Y=None, M=None, g=None, AX=None, mu=1.0, vbound=None, done=None,
               nzero=None, avok=None, rcols=1, sentinel=SENTINEL):
    """One operator application (``ace_linop_host``).

    op: "A" | "AH" | "K" | "G" | "setup"; path: "f64" | "f64_fused" | "i8".  A: (m, n) shared or (batch, m, n)
    private.  Vectors are [batch * rcols][n] (Z, N) / [..][m] (Y, M, g, AX; K and G take their operand in ``g``);
    mu, vbound, done, nzero, avok are per realisation (scalars broadcast).  Returns the output array
    ([batch * rcols][m], AH: [..][n]) with untouched entries equal to ``sentinel (1 + 1j)``; "setup" returns
    (K, G, c) as the operator setup left them.
    """
    A = np.ascontiguousarray(np.asarray(A, dtype=np.complex128))
    shared = A.ndim == 2
    m, n = A.shape[-2:]
    a = LinopArgs()
    a.op, a.path, a.a_shared, a.m, a.n, a.rcols = OPS[op], PATHS[path], int(shared), m, n, int(rcols)
    keep = [A]
    if op == "setup":
        batch = 1 if shared else A.shape[0]
        K = np.zeros((batch, m, m), np.complex128)
        G = np.zeros((batch, m, m), np.complex128)
        c = np.zeros(2)
        mu_a = np.ones(batch)
        a.batch, a.A, a.mu, a.out, a.out2, a.out3 = batch, _ptr(A), _ptr(mu_a), _ptr(K), _ptr(G), _ptr(c)
        check(LIB.ace_linop_host(C.byref(a)))
        return (K[0], G[0], c) if shared else (K, G, c)
    first = next(x for x in (Z, Y, g) if x is not None)
    nv = np.shape(first)[0]
    if nv % rcols:
        raise ValueError("the vector count must be a multiple of rcols")
    batch = nv // rcols
    if not shared and A.shape[0] != batch:
        raise ValueError("one private codebook per realisation")
    Z, N, Y, M = _c(Z, (nv, n)), _c(N, (nv, n)), _c(Y, (nv, m)), _c(M, (nv, m))
    g, AX = _c(g, (nv, m)), _c(AX, (nv, m))
    mu_a = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float64), (batch,)))
    vb = None if vbound is None else np.ascontiguousarray(np.broadcast_to(np.asarray(vbound, np.float64), (batch,)))
    flags = [None if f is None else np.ascontiguousarray(np.broadcast_to(np.asarray(f, np.int32), (batch,)))
             for f in (done, nzero, avok)]
    out = np.empty((nv, n if op == "AH" else m), np.complex128)
    a.batch, a.A = batch, _ptr(A)
    a.Z, a.N, a.Y, a.M, a.g, a.AX = (_ptr(x) for x in (Z, N, Y, M, g, AX))
    a.mu, a.vbound = _ptr(mu_a), _ptr(vb)
    a.done, a.nzero, a.avok = (_ptr(f, _ip) for f in flags)
    a.sentinel, a.out = float(sentinel), _ptr(out)
    keep += [Z, N, Y, M, g, AX, mu_a, vb, flags, out]
    check(LIB.ace_linop_host(C.byref(a)))
    return out


def zgemm_host(mode, conj_l, M, K, nb, L, V, C_, E=None, *, ldl, ldv, ldc, strideL=0, strideV=0, strideC=0, nz=1,
               klim=None, klim_stride=0):
    """The f64 3M GEMM launcher on host arrays (``ace_zgemm_host``): L, V, C_, E flat complex128 arrays; C_ is
    uploaded as given and returned as the kernel left it (a copy)."""
    L = np.ascontiguousarray(np.asarray(L, np.complex128).ravel())
    V = np.ascontiguousarray(np.asarray(V, np.complex128).ravel())
    Cc = np.array(np.asarray(C_, np.complex128).ravel(), copy=True)
    Ee = None if E is None else np.ascontiguousarray(np.asarray(E, np.complex128).ravel())
    if Ee is not None and Ee.size != Cc.size:
        raise ValueError("E and C have one layout")
    kl = None if klim is None else np.ascontiguousarray(np.asarray(klim, np.float64).ravel())
    check(LIB.ace_zgemm_host(int(mode), int(bool(conj_l)), int(M), int(K), int(nb), _ptr(L), L.size, int(ldl),
                             int(strideL), _ptr(V), V.size, int(ldv), int(strideV), _ptr(Cc), _ptr(Ee), Cc.size,
                             int(ldc), int(strideC), int(nz), _ptr(kl), 0 if kl is None else kl.size,
                             int(klim_stride)))
    return Cc
