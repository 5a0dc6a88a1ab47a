"""CPU tests of the unit path's test entry (ace_unit_host) and of its Python mirror (ace_amd.ustep): the argument
checks, which run before any HIP call.  No compute calls -- there is no GPU here."""
import ctypes as C

import numpy as np
import pytest

_dp, _ip, _bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_ubyte)
OPS = ["gyk", "gyf", "ahf", "msr", "ready", "optx"]


def _good(op):
    """Sizes and non-NULL dummy arrays that pass the checks of ``op`` up to the last one (every case below breaks one
    of them, so nothing is dereferenced)."""
    z = np.zeros(4096)
    f = np.zeros(64, np.int32)
    base = dict(batch=2, n=5, m=6, it=3, q=0, rho=1.05, tol_rel=1e-4, tol_abs=1e-8, np=1, waves=8, it_end=9)
    return {
        "gyk": dict(base, A=z, B=z, T=z, Y0=z, M=z, flags=f),                       # use_la = 0: T given
        "gyf": dict(base, A=z, B=z, Y0=z, M=z, Zb1=z, flags=f),
        "ahf": dict(base, A=z, g=z, Zb1=z, flags=f),
        "msr": dict(base, m=256, A=z, B=z, Y0=z, M=z, AX=z, S0=z, flags=f),
        "ready": dict(base, flags=f),
        "optx": dict(base, A=z, Zb1=z, Zb2=z, flags=f),
    }[op]


def _call(op, **kw):
    from ace_amd._lib import LIB, UnitArgs
    from ace_amd.ustep import OPS as TABLE
    a = UnitArgs()
    a.op = TABLE[op] if isinstance(op, str) else op
    keep = []
    for k, v in kw.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data_as(_ip if v.dtype == np.int32 else _dp)
        setattr(a, k, v)
    rc = LIB.ace_unit_host(C.byref(a))
    return rc, LIB.ace_last_error().decode()


def test_the_tables_match_the_header():
    from ace_amd import ustep
    from ace_amd._lib import UnitArgs
    text = (__import__("pathlib").Path(__file__).resolve().parents[1] / "include" / "ace.h").read_text()
    enum = text[text.index("ACE_UNIT_GYK = 0"):text.index("ACE_UNIT_NOPS")]
    names = [t.strip().split(" ")[0] for t in enum.replace("\n", " ").split(",") if t.strip()]
    assert [n[len("ACE_UNIT_"):].lower() for n in names] == OPS == list(ustep.OPS)
    assert f"#define ACE_UNIT_NSTATE {len(ustep.STATE)}\n" in text and f"#define ACE_UNIT_NFLAG {len(ustep.FLAGS)}\n" in text
    listed = text[text.index("state, state_out [batch][ACE_UNIT_NSTATE]:"):text.index("(NULL state: zeros, mu = 1)\n *   flags, flags_out [batch][ACE_UNIT")]
    listed = listed.split(":", 1)[1].replace("*", " ").replace("\n", " ")
    assert [t.strip() for t in listed.split(",") if t.strip()] == list(ustep.STATE)
    listed = text[text.index("flags, flags_out [batch][ACE_UNIT_NFLAG]:"):text.index("done_count / mspcount (and _out)")]
    listed = listed.split(":", 1)[1].replace("*", " ").replace("\n", " ")
    assert [t.strip() for t in listed.split(",") if t.strip()] == list(ustep.FLAGS)
    # the struct's fields, in order, as the header declares them
    body = text[text.index("typedef struct ace_unit_args {"):text.index("} ace_unit_args;")].split("{", 1)[1]
    fields = []
    for decl in body.split(";"):
        for w in ("const", "double", "int32_t", "unsigned", "char", "*"):
            decl = decl.replace(w, " ")
        fields += [t.strip().split("[")[0] for t in decl.split(",") if t.strip()]
    assert fields == [k for k, _ in UnitArgs._fields_]
    # and the control block's fields the entry carries are the ones the issue lists, every one of RealState's unit fields
    common = (__import__("pathlib").Path(__file__).resolve().parents[1] / "2ace-mmwave-channel-estimation_amd" / "csrc"
              / "ace_common.hpp").read_text()
    for k in ustep.FLAGS + tuple(s for s in ustep.STATE if not s.startswith("kf")) + ("kf", "kfcum"):
        assert f" {k}" in common[common.index("struct RealState {"):common.index("static_assert(sizeof(RealState)")], k


def test_null_arguments_and_unknown_ops():
    from ace_amd._lib import LIB, ACE_ERR_ARG
    assert LIB.ace_unit_host(None) == ACE_ERR_ARG and "NULL arguments" in LIB.ace_last_error().decode()
    for op in (-1, len(OPS)):
        rc, msg = _call(op, **_good("gyf"))
        assert rc == ACE_ERR_ARG and "unknown op" in msg


@pytest.mark.parametrize("op", OPS)
def test_every_required_array_is_required_by_name(op):
    from ace_amd._lib import ACE_ERR_ARG
    good = _good(op)
    for name, v in good.items():
        if not isinstance(v, np.ndarray):
            continue
        rc, msg = _call(op, **{k: x for k, x in good.items() if k != name})
        assert rc == ACE_ERR_ARG and f"NULL {name}" in msg and f"({op})" in msg, (name, rc, msg)


def test_the_ping_pong_choice_decides_which_buffer_is_required():
    """Yo = Y[q]; the Z of the previous iterate is Zb1 at odd iterations and Zb2 at even ones; an m-space run from
    `it` reads the buffers of iterate it - 1."""
    from ace_amd._lib import ACE_ERR_ARG
    good = _good("gyf")
    rc, msg = _call("gyf", **{**good, "q": 1})
    assert rc == ACE_ERR_ARG and "NULL Y1" in msg
    rc, msg = _call("gyf", **{**good, "it": 4})
    assert rc == ACE_ERR_ARG and "NULL Zb2" in msg
    rc, msg = _call("gyk", **{**{k: v for k, v in _good("gyk").items() if k != "T"}, "use_la": 1})
    assert rc == ACE_ERR_ARG and "NULL Zb1" in msg                    # apply_A folded in: Z instead of T
    rc, msg = _call("msr", **{**_good("msr"), "it": 4, "it_end": 9})
    assert rc == ACE_ERR_ARG and ("NULL Y1" in msg or "NULL S1" in msg)


@pytest.mark.parametrize("op,name,value", [
    ("gyk", "batch", 0), ("gyf", "batch", -3), ("msr", "batch", 0), ("ready", "batch", 0), ("optx", "batch", 0),
    ("gyk", "m", 0), ("gyf", "m", -1), ("ahf", "m", 0), ("optx", "m", 0), ("gyk", "n", 0), ("gyf", "n", -2),
    ("gyf", "guard", -1), ("gyk", "rho", 0.0), ("gyf", "rho", -1.05), ("msr", "rho", 0.0), ("ahf", "rho", float("nan")),
    ("gyk", "it", 0), ("gyf", "it", -4), ("msr", "it", 0), ("ready", "it", 0), ("gyf", "q", 2), ("gyk", "q", -1),
    ("gyf", "np", 5), ("gyf", "np", -1), ("msr", "it_end", 3), ("msr", "it_end", 0), ("msr", "waves", 2), ("msr", "waves", 0)])
def test_bad_sizes_are_argument_errors(op, name, value):
    from ace_amd._lib import ACE_ERR_ARG
    rc, msg = _call(op, **{**_good(op), name: value})
    assert rc == ACE_ERR_ARG and name in msg and f"({op})" in msg, (rc, msg)


@pytest.mark.parametrize("op", [o for o in OPS if o != "msr"])
def test_more_than_256_rows_is_unsupported(op):
    from ace_amd._lib import ACE_ERR_ARG, ACE_ERR_UNSUPPORTED
    rc, msg = _call(op, **{**_good(op), "m": 257})
    assert rc == ACE_ERR_UNSUPPORTED and "m = 257" in msg
    # 256 passes the size check (and stops at the NULL operand: nothing is launched)
    rc, msg = _call(op, **{**_good(op), "m": 256, "flags": None})
    assert rc == ACE_ERR_ARG and "NULL flags" in msg


@pytest.mark.parametrize("m", [1, 64, 255])
def test_the_run_takes_256_rows_only(m):
    from ace_amd._lib import ACE_ERR_UNSUPPORTED
    rc, msg = _call("msr", **{**_good("msr"), "m": m})
    assert rc == ACE_ERR_UNSUPPORTED and f"m = {m}" in msg and "(msr)" in msg


def test_python_mirror_refuses_bad_shapes_before_the_call():
    import ace_amd
    from ace_amd import ustep
    assert ace_amd.ustep is ustep and not hasattr(ace_amd, "unit_host")
    z = np.zeros
    with pytest.raises(ValueError, match="unknown op"):
        ustep.unit_host("nope", batch=1, n=4, m=3)
    with pytest.raises(TypeError, match="unknown ace_unit_args field"):
        ustep.unit_host("gyf", batch=1, n=4, m=3, nonsense=z(3))
    with pytest.raises(ValueError, match="at most 4"):
        ustep.unit_host("gyf", batch=1, n=4, m=3, fl=(0.1,) * 5)
    for kw in (dict(A=z((3, 5))), dict(A=z((3, 4)), B=z((2, 4))), dict(A=z((3, 4)), Y0=z((2, 4))),
               dict(A=z((3, 4)), Zb1=z((2, 3))), dict(A=z((3, 4)), state=z((2, 3))),
               dict(A=z((3, 4)), rank_one=z(3, np.uint8))):
        with pytest.raises(ValueError, match="expected shape"):
            ustep.unit_host("gyf", batch=2, n=4, m=3, **kw)
    # the C checks reach Python as AceError with the argument's name
    fl = ustep.flags_array(2)
    with pytest.raises(ace_amd.AceError, match="NULL B"):          # (state may be NULL: zeros, mu = 1)
        ustep.unit_host("gyf", batch=2, n=4, m=3, A=z((3, 4)), flags=fl)
    with pytest.raises(ace_amd.AceError, match="rho"):
        ustep.unit_host("gyk", batch=1, n=4, m=3, rho=0.0)
    with pytest.raises(ace_amd.AceError, match="m = 300"):
        ustep.unit_host("optx", batch=1, n=4, m=300)
    with pytest.raises(ace_amd.AceError, match="it_end"):
        ustep.unit_host("msr", batch=1, n=4, m=256, it=5, it_end=5)
    s, f = ustep.state_array(3, mu=[1, 2, 3], fs0=0.5), ustep.flags_array(3, done=[0, 1, 0])
    assert s[:, 0].tolist() == [1, 2, 3] and (s[:, ustep.STATE.index("fs0")] == 0.5).all()
    assert f[:, ustep.FLAGS.index("done")].tolist() == [0, 1, 0] and f.dtype == np.int32
    assert s.shape == (3, len(ustep.STATE)) and f.shape == (3, len(ustep.FLAGS))
