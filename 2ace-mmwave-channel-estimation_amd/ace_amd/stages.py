"""Host-side mirror of the stage test entry ``ace_stage_host`` (include/ace.h).

One kernel of the r-column stages or of the pipeline around them (csrc/ace_stage.hip) through the launcher a solve
calls: init and Y-step at r columns, opt_X / opt_Y, the rotation by the eigenvectors of ``X^H X``, test quality, best
of restarts, rollback and rescale, the per-realisation partitions' Schur form, and the small movers and norms.  For
tests (tests/test_gpu_stage.py); no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import LIB, StageArgs, check

OPS = {k: i for i, k in enumerate(
    ["init_r", "ystep_r", "finalize_r", "gram_rotate", "quality", "part_quality", "keep_best", "finish", "part_geinv",
     "part_gfix", "part_expand", "part_compact", "anorm", "bnorm", "gather_rows", "gather_b", "move_rows", "move_bytes",
     "put_col", "flag_bits", "fill"])}
STATE = ("mu", "last_res", "opt_obj", "nB", "obj2", "nAX2", "nY2", "nJM2", "dY2")
FLAGS = ("iters", "done", "status", "objcol", "optsrc", "optysrc")
PART_MAXTE = 96
RMAX = 32

SENTINEL = -7.25e77     # default fill of the f64 / c128 outputs (both components)
ISENTINEL = 0x5A5A5A5A  # ... of the int32 outputs (byte outputs: 0x5A)

_dp, _ip, _bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_ubyte)
_CPLX = {"X", "Y", "P0", "S", "g", "M", "A", "G", "geinv", "Xmax", "Ymax", "optX", "optY", "Zb1", "Zb2", "Yb1", "Yb2"}
_REAL = {"B", "q", "qmax", "anorm", "bnorm", "src", "state"}
_INT = {"flags", "rows", "idx", "isrc", "idst"}
_BYTE = {"mask", "bsrc"}
_SCALARS = {"row_mode", "batch", "n", "m", "r", "nc", "mt", "count", "ld", "col", "first", "scatter", "or_mask", "bit",
            "len", "mu0", "tol_abs", "value"}


def state_array(batch, **kw):
    """[batch][len(STATE)] f64 control-block values: mu = 1 and zeros except the given fields (scalars broadcast)."""
    s = np.zeros((batch, len(STATE)))
    s[:, 0] = 1.0
    for k, v in kw.items():
        s[:, STATE.index(k)] = v
    return s


def flags_array(batch, **kw):
    """[batch][len(FLAGS)] int32 control-block flags: zeros except the given fields."""
    f = np.zeros((batch, len(FLAGS)), np.int32)
    for k, v in kw.items():
        f[:, FLAGS.index(k)] = v
    return f


def _shape(x, shape, name):
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(x.shape)}")
    return x


def _sizes(kw, *names):
    out = []
    for k in names:
        if k not in kw:
            raise ValueError(f"missing size {k}")
        out.append(int(kw[k]))
    return out


def _outputs(op, kw):
    """{field: (shape, dtype)} of the outputs of ``op`` at the sizes in kw (the table of include/ace.h)."""
    g = lambda *names: _sizes(kw, *names)   # noqa: E731
    c, f, i, u = np.complex128, np.float64, np.int32, np.uint8
    if op == "init_r":
        b, n, m, r = g("batch", "n", "m", "r")
        return {"Xo": ((b, r, n), c), "No": ((b, r, n), c), "Yo": ((b, r, m), c), "Mo": ((b, r, m), c),
                "state_out": ((b, len(STATE)), f), "flags_out": ((b, len(FLAGS)), i)}
    if op == "ystep_r":
        b, m, r = g("batch", "m", "r")
        return {"Yo": ((b, r, m), c), "Mo": ((b, r, m), c), "state_out": ((b, len(STATE)), f),
                "flags_out": ((b, len(FLAGS)), i)}
    if op == "finalize_r":
        b, n, m, nc = g("batch", "n", "m", "nc")
        return {"Xo": ((b, nc, n), c), "Yo": ((b, nc, m), c), "qo": ((b,), f), "iout": ((b, 2), i)}
    if op == "gram_rotate":
        b, n, r = g("batch", "n", "r")
        return {"Xo": ((b, r, n), c), "iout": ((b,), i)}
    if op in ("quality", "part_quality"):
        return {"qo": ((g("batch")[0],), f)}
    if op == "keep_best":
        b, n, m = g("batch", "n", "m")
        return {"qo": ((b,), f), "Xo": ((b, n), c), "Yo": ((b, m), c)}
    if op == "finish":
        b, n, m = g("batch", "n", "m")
        return {"Xo": ((b, n), c), "Yo": ((b, m), c), "iout": ((b,), i)}
    if op == "part_geinv":
        b, m, mt = g("batch", "m", "mt")
        return {"Xo": ((b, m - mt, m - mt), c), "iout": ((b,), i)}
    if op == "part_gfix":
        b, m, r = g("batch", "m", "r")
        return {"Yo": ((b, r, m), c)}
    if op in ("part_expand", "part_compact"):
        b, m, mt, r = g("batch", "m", "mt", "r")
        return {"Yo": ((b, r, m if op == "part_expand" else mt), c)}
    if op == "anorm":
        return {"qo": ((1,), f)}
    if op == "bnorm":
        b, m = g("batch", "m")
        return {"qo": ((b,), f), "Xo": ((b, m), f)}
    if op == "gather_rows":
        cnt, n = g("count", "n")
        return {"Xo": ((cnt, n), c)}
    if op == "gather_b":
        b, cnt = g("batch", "count")
        return {"qo": ((b, cnt), f)}
    if op in ("move_rows", "move_bytes"):
        cnt, ln, m, sc = g("count", "len", "m", "scatter")
        return {("qo" if op == "move_rows" else "bout"): ((m if sc else cnt, ln), f if op == "move_rows" else u)}
    if op == "put_col":
        m, ld = g("m", "ld")
        return {"iout": ((m, ld), i)}
    if op == "flag_bits":
        return {"iout": ((g("m")[0],), i)}
    if op == "fill":
        return {"qo": ((g("m")[0],), f)}
    raise ValueError(f"unknown op {op!r}")


def stage_host(op, *, sentinel=SENTINEL, isentinel=ISENTINEL, **kw):
    """One launcher call (``ace_stage_host``).  ``kw``: the sizes and input arrays of the op under the field names of
    ``ace_stage_args`` (see include/ace.h for which op takes which).  Returns {output field: array}; entries a kernel
    left alone hold ``sentinel`` (c128: in both components) / ``isentinel``."""
    if op not in OPS:
        raise ValueError(f"unknown op {op!r}")
    outs = _outputs(op, kw)
    _check_shapes(op, kw)
    a = StageArgs()
    a.op, a.sentinel, a.isentinel = OPS[op], float(sentinel), int(isentinel)
    keep = []
    for k, v in kw.items():
        if k in _SCALARS:
            setattr(a, k, float(v) if k in ("mu0", "tol_abs", "value") else int(v))
            continue
        if v is None:
            continue
        if k in _CPLX:
            x = np.ascontiguousarray(np.asarray(v, np.complex128))
            p = x.view(np.float64).ctypes.data_as(_dp) if x.size else None
        elif k in _REAL:
            x = np.ascontiguousarray(np.asarray(v, np.float64))
            p = x.ctypes.data_as(_dp)
        elif k in _INT:
            x = np.ascontiguousarray(np.asarray(v, np.int32))
            p = x.ctypes.data_as(_ip)
        elif k in _BYTE:
            x = np.ascontiguousarray(np.asarray(v, np.uint8))
            p = x.ctypes.data_as(_bp)
        else:
            raise TypeError(f"unknown ace_stage_args field {k!r}")
        keep.append(x)
        setattr(a, k, p)
    out = {}
    for k, (shape, dt) in outs.items():
        x = np.empty(shape, dt)
        out[k] = x
        if x.size:
            tp = {np.int32: _ip, np.uint8: _bp}.get(dt, _dp)
            setattr(a, k, (x.view(np.float64) if dt == np.complex128 else x).ctypes.data_as(tp))
    check(LIB.ace_stage_host(C.byref(a)))
    return out


def _check_shapes(op, kw):
    """The array shapes ``ace_stage_host`` cannot see (it takes pointers): ValueError before the call."""
    get = lambda k: None if kw.get(k) is None else np.asarray(kw[k])   # noqa: E731
    sz = {k: int(kw[k]) for k in ("batch", "n", "m", "r", "nc", "mt", "count", "len", "ld") if k in kw}
    b, n, m, r = sz.get("batch", 1), sz.get("n", 1), sz.get("m", 1), sz.get("r", 1)
    nc, mt, cnt, ln = sz.get("nc", 1), sz.get("mt", m), sz.get("count", 0), sz.get("len", 1)
    te, sc = m - mt, int(kw.get("scatter", 0))
    want = {
        "init_r": {"X": (b, r, n), "P0": (b, r, m), "B": (b, m), "mask": (b, m)},
        "ystep_r": {"S": (b, r, m), "g": (b, r, m), "M": (b, r, m), "Y": (b, r, m), "B": (b, m), "mask": (b, m)},
        "finalize_r": {"optX": (b, nc, n), "optY": (b, nc, m), "X": (b, r, n), "Y": (b, r, m), "Zb1": (b, nc, n),
                       "Zb2": (b, nc, n), "Yb1": (b, nc, m), "Yb2": (b, nc, m)},
        "gram_rotate": {"X": (b, r, n), "idst": (b,)},
        "quality": {"A": (cnt, n), "X": (b, n), "B": (b, cnt)},
        "part_quality": {"A": (m, n), "X": (b, n), "B": (b, m), "rows": (b, m)},
        "keep_best": {"q": (b,), "qmax": (b,), "X": (b, n), "Y": (b, m), "Xmax": (b, n), "Ymax": (b, m)},
        "finish": {"q": (b,), "X": (b, n), "Y": (b, m), "Xmax": (b, n), "Ymax": (b, mt), "anorm": (1,), "bnorm": (b,),
                   "idst": (b,)},
        "part_geinv": {"G": (m, m), "rows": (b, m), "idst": (b,)},
        "part_gfix": {"G": (m, m), "geinv": (b, te, te), "g": (b, r, m), "rows": (b, m), "mask": (b, m)},
        "part_expand": {"Y": (b, r, mt), "rows": (b, m)},
        "part_compact": {"Y": (b, r, m), "rows": (b, m)},
        "anorm": {"A": (m, n)},
        "bnorm": {"B": (b, m)},
        "gather_rows": {"A": (m, n), "idx": (cnt,), "anorm": (1,)},
        "gather_b": {"B": (b, m), "idx": (cnt,)},
        "move_rows": {"src": (cnt if sc else m, ln), "idx": (cnt,)},
        "move_bytes": {"bsrc": (cnt if sc else m, ln), "idx": (cnt,)},
        "put_col": {"isrc": (cnt,), "idx": (cnt,), "idst": (m, sz.get("ld", 1))},
        "flag_bits": {"bsrc": (cnt,), "idst": (m,)},
        "fill": {},
    }[op]
    for k, shape in want.items():
        x = get(k)
        if x is not None:
            _shape(x, shape, f"{op}: {k}")
    for k, width in (("state", len(STATE)), ("flags", len(FLAGS))):
        x = get(k)
        if x is not None:
            _shape(x, (b, width), f"{op}: {k}")
    if r > RMAX:
        raise ValueError(f"{op}: r = {r} > {RMAX}")
    if te > PART_MAXTE and op.startswith("part_"):
        raise ValueError(f"{op}: m - mt = {te} test rows, the kernels take {PART_MAXTE}")
