"""CPU tests of the m-space iteration's test entry (ace_nms_host) and of its Python mirror (ace_amd.nms): the argument
checks, which run before any HIP call.  No compute calls -- there is no GPU here."""
import ctypes as C

import numpy as np
import pytest

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
OPS = ["init", "step", "fin", "out"]


def _good(op):
    """Sizes and non-NULL dummy arrays that pass the checks of ``op`` up to the last one (every case below breaks one
    of them, so nothing is dereferenced)."""
    z = np.zeros(4096)
    f = np.zeros(64, np.int32)
    base = dict(batch=2, n=5, m=6, it=1, rho=1.05, tol_rel=1e-4, tol_abs=1e-8)
    return {
        "init": dict(base, Xinit=z, P0=z),
        "step": dict(base, G=z, K=z, Yo=z, M=z, B=z, Eo=z, AEo=z, state=z, flags=f),
        "fin": dict(base, K=z, Yo=z, Yn=z, state=z, flags=f),
        "out": dict(base, Xinit=z, state=z, optW=z, curW=z),
    }[op]


def _call(op, **kw):
    from ace_amd._lib import LIB, NmsArgs
    from ace_amd.nms import OPS as TABLE
    a = NmsArgs()
    a.op = TABLE[op] if isinstance(op, str) else op
    keep = []
    for k, v in kw.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data_as(_ip if v.dtype == np.int32 else _dp)
        setattr(a, k, v)
    rc = LIB.ace_nms_host(C.byref(a))
    return rc, LIB.ace_last_error().decode()


def test_the_tables_match_the_header():
    from ace_amd import nms
    from ace_amd._lib import NmsArgs
    text = (__import__("pathlib").Path(__file__).resolve().parents[1] / "include" / "ace.h").read_text()
    enum = text[text.index("ACE_NMS_INIT = 0"):text.index("ACE_NMS_NOPS")]
    names = [t.strip().split(" ")[0] for t in enum.replace("\n", " ").split(",") if t.strip()]
    assert [n[len("ACE_NMS_"):].lower() for n in names] == OPS == list(nms.OPS)
    assert f"#define ACE_NMS_NSTATE {len(nms.STATE)}\n" in text and f"#define ACE_NMS_NFLAG {len(nms.FLAGS)}\n" in text
    listed = text[text.index("state, state_out [batch][ACE_NMS_NSTATE]:"):text.index("(NULL state: zeros")]
    listed = listed.split(":", 1)[1].replace("*", " ").replace("\n", " ")
    assert [t.strip() for t in listed.split(",") if t.strip()] == list(nms.STATE)
    # the struct's fields, in order, as the header declares them
    body = text[text.index("typedef struct ace_nms_args {"):text.index("} ace_nms_args;")].split("{", 1)[1]
    fields = []
    for decl in body.split(";"):
        decl = decl.replace("const", " ").replace("double", " ").replace("int32_t", " ").replace("*", " ")
        fields += [t.strip() for t in decl.split(",") if t.strip()]
    assert fields == [k for k, _ in NmsArgs._fields_]


def test_null_arguments_and_unknown_ops():
    from ace_amd._lib import LIB, ACE_ERR_ARG
    assert LIB.ace_nms_host(None) == ACE_ERR_ARG and "NULL arguments" in LIB.ace_last_error().decode()
    for op in (-1, len(OPS)):
        rc, msg = _call(op, **_good("step"))
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


@pytest.mark.parametrize("op,name,value", [
    ("init", "batch", 0), ("step", "batch", -3), ("fin", "batch", 0), ("out", "batch", 0),
    ("init", "m", 0), ("step", "m", -1), ("fin", "m", 0), ("out", "m", 0), ("init", "n", 0), ("step", "n", -2),
    ("step", "guard", -1), ("step", "rho", 0.0), ("step", "rho", -1.05), ("fin", "rho", 0.0),
    ("step", "rho", float("nan")), ("step", "it", 0), ("step", "it", -4)])
def test_bad_sizes_are_argument_errors(op, name, value):
    from ace_amd._lib import ACE_ERR_ARG
    rc, msg = _call(op, **{**_good(op), name: value})
    assert rc == ACE_ERR_ARG and name in msg and f"({op})" in msg, (rc, msg)


def test_fin_and_out_take_any_iteration_number():
    """`it` is the step's: fin and out pass that check (and stop at the one after it)."""
    from ace_amd._lib import ACE_ERR_ARG
    for op, drop in (("fin", "K"), ("out", "optW")):
        good = _good(op)
        rc, msg = _call(op, **{**{k: v for k, v in good.items() if k != drop}, "it": 0})
        assert rc == ACE_ERR_ARG and f"NULL {drop}" in msg


@pytest.mark.parametrize("op", OPS)
def test_more_than_256_rows_is_unsupported(op):
    from ace_amd._lib import ACE_ERR_ARG, ACE_ERR_UNSUPPORTED
    rc, msg = _call(op, **{**_good(op), "m": 257})
    assert rc == ACE_ERR_UNSUPPORTED and "m = 257" in msg
    # 256 passes the size check (and stops at the NULL operand: nothing is launched)
    rc, msg = _call(op, **{**_good(op), "m": 256, "Xinit": None, "K": None})
    assert rc == ACE_ERR_ARG and "NULL" in msg


def test_python_mirror_refuses_bad_shapes_before_the_call():
    import ace_amd
    from ace_amd import nms
    assert ace_amd.nms is nms and not hasattr(ace_amd, "nms_host")
    z = np.zeros
    with pytest.raises(ValueError, match="unknown op"):
        nms.nms_host("nope", batch=1, n=4, m=3)
    with pytest.raises(TypeError, match="unknown ace_nms_args field"):
        nms.nms_host("fin", batch=1, n=4, m=3, nonsense=z(3))
    for kw in (dict(Xinit=z((2, 5)), P0=z((2, 3))),                # Xinit is not [b][n]
               dict(Xinit=z((2, 4)), P0=z((2, 4))),                # P0 is not [b][m]
               dict(Xinit=z((2, 4)), P0=z((2, 3)), state=z((2, 3)))):
        with pytest.raises(ValueError, match="expected shape"):
            nms.nms_host("init", batch=2, n=4, m=3, **kw)
    # the C checks reach Python as AceError with the argument's name
    with pytest.raises(ace_amd.AceError, match="NULL P0"):
        nms.nms_host("init", batch=2, n=4, m=3, Xinit=z((2, 4)))
    with pytest.raises(ace_amd.AceError, match="rho"):
        nms.nms_host("fin", batch=1, n=4, m=3, rho=0.0)
    with pytest.raises(ace_amd.AceError, match="m = 300"):
        nms.nms_host("out", batch=1, n=4, m=300)
    s, f = nms.state_array(3, mu=[1, 2, 3], nep2=0.5), nms.flags_array(3, done=[0, 1, 0])
    assert s[:, 0].tolist() == [1, 2, 3] and (s[:, nms.STATE.index("nep2")] == 0.5).all()
    assert f[:, nms.FLAGS.index("done")].tolist() == [0, 1, 0] and f.dtype == np.int32
    assert s.shape == (3, len(nms.STATE)) and f.shape == (3, len(nms.FLAGS))
