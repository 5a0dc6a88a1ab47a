"""CPU tests of the private code-image kernels' test entry (ace_pc_host) and of its Python mirror (ace_amd.pcode):
the argument checks, which run before any HIP call.  No compute calls -- there is no GPU here."""
import ctypes as C

import numpy as np
import pytest

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
OPS = ["pack", "kmat", "inv", "tiles", "apply_a", "step"]


def _good(op):
    """Sizes and non-NULL dummy arrays that pass the checks of ``op`` up to the last one (every case below breaks one
    of them, so nothing is dereferenced but the state's mu)."""
    z = np.ones(4096)
    f = np.zeros(64, np.int32)
    base = dict(batch=2, m=6, n=5)
    return {
        "pack": dict(base, A=z),
        "kmat": dict(base, A=z),
        "inv": dict(base, Gin=z),
        "tiles": dict(base, Gin=z),
        "apply_a": dict(base, A=z, X0=z),
        "step": dict(base, A=z, B=z, Yo=z, M=z, Z=z, N=z, state=z, flags=f),
    }[op]


def _call(op, **kw):
    from ace_amd._lib import LIB, PcArgs
    from ace_amd.pcode import OPS as TABLE
    a = PcArgs()
    a.op = TABLE[op] if isinstance(op, str) else op
    keep = []
    for k, v in kw.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data_as(_ip if v.dtype == np.int32 else _dp)
        setattr(a, k, v)
    rc = LIB.ace_pc_host(C.byref(a))
    return rc, LIB.ace_last_error().decode()


def test_the_tables_match_the_header():
    from ace_amd import pcode
    from ace_amd._lib import PcArgs
    text = (__import__("pathlib").Path(__file__).resolve().parents[1] / "include" / "ace.h").read_text()
    enum = text[text.index("ACE_PC_PACK = 0"):text.index("ACE_PC_NOPS")]
    names = [t.strip().split(" ")[0] for t in enum.replace("\n", " ").split(",") if t.strip()]
    assert [n[len("ACE_PC_"):].lower() for n in names] == OPS == list(pcode.OPS)
    forms = text[text.index("ACE_PC_SCHUR = 0"):text.index("ACE_PC_NFORMS")]
    names = [t.strip().split(" ")[0] for t in forms.replace("\n", " ").split(",") if t.strip()]
    assert [n[len("ACE_PC_"):].lower() for n in names] == list(pcode.FORMS)
    assert f"#define ACE_PC_NSTATE {len(pcode.STATE)}\n" in text
    assert f"#define ACE_PC_NFLAG {len(pcode.FLAGS)}\n" in text
    for head, stop, table in (
            ("state, state_out [batch][ACE_PC_NSTATE]:", "flags, flags_out [batch][ACE_PC_NFLAG]", pcode.STATE),
            ("flags, flags_out [batch][ACE_PC_NFLAG]:", "guard_ok: 1 when", pcode.FLAGS)):
        listed = text[text.index(head):]
        listed = listed[:listed.index(stop, 10)].split(":", 1)[1].replace("*", " ").replace("\n", " ")
        assert [t.strip() for t in listed.split(",") if t.strip()] == list(table)
    # the struct's fields, in order, as the header declares them
    body = text[text.index("typedef struct ace_pc_args {"):text.index("} ace_pc_args;")].split("{", 1)[1]
    fields = []
    for decl in body.split(";"):
        for w in ("const", "double", "uint32_t", "int32_t", "*"):
            decl = decl.replace(w, " ")
        fields += [t.strip() for t in decl.split(",") if t.strip()]
    assert fields == [k for k, _ in PcArgs._fields_]


def test_the_sizes_match_the_kernels_dimensions():
    """pcode.dims restates pc_dims: checked against the formulas written out in the source."""
    from ace_amd import pcode
    for m, n in ((1, 1), (17, 100), (256, 2048), (129, 129)):
        d = pcode.dims(m, n)
        assert d["mt"] == -(-m // 16) and d["mp32"] == 32 * -(-m // 32) and d["ntile"] == d["mt"] * (d["mt"] + 1) // 2
        assert d["nH"] == -(-n // 16) * -(-d["mt"] // 8) * 128 and d["nA"] == d["mt"] * -(-(-(-n // 16)) // 8) * 128
        assert d["nR"] == m * -(-n // 16)


def test_null_arguments_and_unknown_ops_and_forms():
    from ace_amd._lib import LIB, ACE_ERR_ARG
    assert LIB.ace_pc_host(None) == ACE_ERR_ARG and "NULL arguments" in LIB.ace_last_error().decode()
    for op in (-1, len(OPS)):
        rc, msg = _call(op, **_good("step"))
        assert rc == ACE_ERR_ARG and "unknown op" in msg
    for form in (-1, 2):
        rc, msg = _call("inv", **{**_good("inv"), "form": form})
        assert rc == ACE_ERR_ARG and "unknown form" in msg and "(inv)" in msg
    # the other operations do not read the form
    rc, msg = _call("tiles", batch=2, m=6, n=5, form=7)
    assert rc == ACE_ERR_ARG and "NULL Gin" in msg


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
    ("pack", "batch", 0), ("kmat", "batch", -3), ("inv", "batch", 0), ("tiles", "batch", 0), ("apply_a", "batch", 0),
    ("step", "batch", 0), ("pack", "m", 0), ("kmat", "m", -1), ("inv", "m", 0), ("tiles", "m", 0), ("apply_a", "m", 0),
    ("step", "m", 0), ("pack", "n", 0), ("kmat", "n", -2), ("apply_a", "n", 0), ("step", "n", 0),
    ("pack", "guard", -1), ("step", "guard", -1), ("step", "yn_id", 3), ("step", "yn_id", -1)])
def test_bad_sizes_are_argument_errors(op, name, value):
    from ace_amd._lib import ACE_ERR_ARG
    rc, msg = _call(op, **{**_good(op), name: value})
    assert rc == ACE_ERR_ARG and name in msg and f"({op})" in msg, (rc, msg)


@pytest.mark.parametrize("mu", [0.0, -1.0, float("nan")])
def test_a_step_needs_a_positive_mu_in_every_realisation(mu):
    from ace_amd._lib import ACE_ERR_ARG
    from ace_amd.pcode import STATE
    s = np.ones(4096)
    s[len(STATE)] = mu   # realisation 1
    rc, msg = _call("step", **{**_good("step"), "state": s})
    assert rc == ACE_ERR_ARG and "mu" in msg and "realisation 1" in msg and "(step)" in msg, (rc, msg)


@pytest.mark.parametrize("op", OPS)
def test_sizes_beyond_the_kernels_are_unsupported(op):
    from ace_amd._lib import ACE_ERR_ARG, ACE_ERR_UNSUPPORTED
    rc, msg = _call(op, **{**_good(op), "m": 257})
    assert rc == ACE_ERR_UNSUPPORTED and "m = 257" in msg
    rc, msg = _call(op, **{**_good(op), "n": 2049})
    assert rc == ACE_ERR_UNSUPPORTED and "n = 2049" in msg
    # 256 x 2048 passes the size checks (and stops at the NULL operand: nothing is launched)
    rc, msg = _call(op, **{**_good(op), "m": 256, "n": 2048, "A": None, "Gin": None})
    assert rc == ACE_ERR_ARG and "NULL" in msg


def test_python_mirror_refuses_bad_shapes_before_the_call():
    import ace_amd
    from ace_amd import pcode
    assert ace_amd.pcode is pcode and not hasattr(ace_amd, "pc_host")
    z = np.zeros
    with pytest.raises(ValueError, match="unknown op"):
        pcode.pc_host("nope", batch=1, m=3, n=4)
    with pytest.raises(ValueError, match="unknown form"):
        pcode.pc_host("inv", batch=1, m=3, form="lu")
    with pytest.raises(TypeError, match="unknown ace_pc_args field"):
        pcode.pc_host("step", batch=1, m=3, n=4, nonsense=z(3))
    for kw in (dict(A=z((2, 3, 5))),                                # A is not [b][m][n]
               dict(A=z((2, 3, 4)), X0=z((2, 3))),                  # X0 is not [b][n]
               dict(A=z((2, 3, 4)), X0=z((2, 4)), Yo=z((2, 4)))):   # Yo is not [b][m]
        with pytest.raises(ValueError, match="expected shape"):
            pcode.pc_host("apply_a", batch=2, m=3, n=4, **kw)
    with pytest.raises(ValueError, match="expected shape"):
        pcode.pc_host("inv", batch=1, m=33, Gin=z((1, 33, 33)))     # the setup's frame is mp32 x mp32
    # the C checks reach Python as AceError with the argument's name
    with pytest.raises(ace_amd.AceError, match="NULL X0"):
        pcode.pc_host("apply_a", batch=2, m=3, n=4, A=z((2, 3, 4)))
    with pytest.raises(ace_amd.AceError, match="m = 300"):
        pcode.pc_host("tiles", batch=1, m=300)
    s, f = pcode.state_array(3, mu=[1, 2, 3], vbound=0.5), pcode.flags_array(3, done=[0, 1, 0])
    assert s[:, 0].tolist() == [1, 2, 3] and (s[:, pcode.STATE.index("vbound")] == 0.5).all()
    assert f[:, pcode.FLAGS.index("done")].tolist() == [0, 1, 0] and f.dtype == np.int32
    assert s.shape == (3, len(pcode.STATE)) and f.shape == (3, len(pcode.FLAGS))
