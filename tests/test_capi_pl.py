"""CPU tests of the PhaseLift step kernels' test entry (ace_pl_host) and of its Python mirror (ace_amd.plstep): the
argument checks, which run before any HIP call.  No compute calls -- there is no GPU here."""
import ctypes as C
import pathlib

import numpy as np
import pytest

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
OPS = ["init", "outer_begin", "theta", "make_y", "set_ay", "grad", "gy", "prox_in", "assemble", "zasm", "take_z",
       "apply_a", "make_x", "set_ax", "backtrack", "iterate", "chol", "transpose", "final_vec", "outputs"]
# the arrays each operation requires (include/ace.h)
NEED = {
    "init": ["bvec"],
    "outer_begin": ["x", "z", "Ax", "Az", "state"],
    "theta": ["state", "cnt"],
    "make_y": ["xo", "zo", "state", "act"],
    "set_ay": ["Axo", "Azo", "Aex", "state", "act"],
    "grad": ["Ay", "bvec", "gAy", "R", "state", "act"],
    "gy": ["R", "Pg"],
    "prox_in": ["zo", "G", "state", "act"],
    "assemble": ["V", "lam", "misc", "tau", "state", "act"],
    "zasm": ["VT", "P", "misc"],
    "take_z": ["Znew", "zo", "G", "misc", "tau", "state", "act"],
    "apply_a": ["x", "R", "RT", "act"],
    "make_x": ["xo", "z", "y", "G", "Axo", "Az", "state", "act", "cnt"],
    "set_ax": ["Aex", "state", "act"],
    "backtrack": ["Ax", "Ay", "bvec", "gAy", "state", "act"],
    "iterate": ["x", "Ax", "gAx", "state", "cnt"],
    "chol": ["K"],
    "transpose": ["R"],
    "final_vec": ["x", "V1", "lam"],
    "outputs": ["state"],
}
INTS = ("act", "cnt", "ok", "iters", "status")


def _good(op):
    """Sizes and non-NULL dummy arrays that pass the checks of ``op`` (every case below breaks one of them, so
    nothing is dereferenced)."""
    z, f = np.ones(4096), np.zeros(64, np.int32)
    return dict(dict(batch=2, m=6, d=5), **{k: (f if k in INTS else z) for k in NEED[op]})


def _call(op, **kw):
    from ace_amd._lib import LIB, PlArgs
    from ace_amd.plstep import OPS as TABLE
    a = PlArgs()
    a.op = TABLE[op] if isinstance(op, str) else op
    keep = []
    for k, v in kw.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data_as(_ip if v.dtype == np.int32 else _dp)
        setattr(a, k, v)
    rc = LIB.ace_pl_host(C.byref(a))
    return rc, LIB.ace_last_error().decode()


def test_the_tables_match_the_header_and_the_struct():
    from ace_amd import plstep
    from ace_amd._lib import PlArgs
    import pl_cases
    import pl_ref
    root = pathlib.Path(__file__).resolve().parents[1]
    text = (root / "include" / "ace.h").read_text()
    enum = text[text.index("ACE_PL_INIT = 0"):text.index("ACE_PL_NOPS")]
    names = [t.strip().split(" ")[0] for t in enum.replace("\n", " ").split(",") if t.strip()]
    assert [n[len("ACE_PL_"):].lower() for n in names] == OPS == list(plstep.OPS)
    assert f"#define ACE_PL_NSTATE {len(plstep.STATE)}\n" in text
    assert f"#define ACE_PL_ISENTINEL {plstep.ISENTINEL:#X}\n".replace("0X", "0x") in text
    listed = text[text.index("state, state_out [batch][ACE_PL_NSTATE]:"):]
    listed = listed[:listed.index("(PlState in field order")].split(":", 1)[1].replace("*", " ").replace("\n", " ")
    assert [t.strip() for t in listed.split(",") if t.strip()] == list(plstep.STATE) == list(pl_ref.STATE)
    # PlState's own field order (csrc/ace_phaselift.hpp)
    hpp = (root / "2ace-mmwave-channel-estimation_amd" / "csrc" / "ace_phaselift.hpp").read_text()
    body = hpp[hpp.index("struct PlState {"):hpp.index("struct PlArgs")].split("{", 1)[1].split("}")[0]
    fields = []
    for line in body.split("\n"):
        decl = line.split("//")[0]
        for w in ("double", "int32_t", ";"):
            decl = decl.replace(w, " ")
        fields += [t.strip() for t in decl.split(",") if t.strip()]
    assert fields[:len(plstep.STATE)] == list(plstep.STATE) and fields[len(plstep.STATE):] == ["pad[3]"]
    assert plstep.NFLOAT == fields.index("n_iter")
    # the struct's fields, in order, as the header declares them
    body = text[text.index("typedef struct ace_pl_args {"):text.index("} ace_pl_args;")].split("{", 1)[1]
    fields = []
    for decl in body.split(";"):
        for w in ("const", "double", "uint32_t", "int32_t", "*"):
            decl = decl.replace(w, " ")
        fields += [t.strip() for t in decl.split(",") if t.strip()]
    assert fields == [k for k, _ in PlArgs._fields_]
    # the header's list of what each operation needs is what the entry enforces (test below) and what NEED says
    for op in OPS:
        line = text[text.index(f"ACE_PL_{op.upper()} "):]
        line = line[:line.index("->")]
        for k in NEED[op]:
            assert k in line.replace(",", " ").replace(":", " ").replace("(", " ").split(), (op, k)
    assert plstep.shapes(3, 7, 5) == pl_cases.shapes(3, 7, 5)
    assert {k: v for k, v in pl_ref.PARAMS.items() if k != "lam_reg"} == \
        {k: v for k, v in plstep.PARAMS.items() if k != "lambda"}
    assert pl_ref.PARAMS["lam_reg"] == plstep.PARAMS["lambda"]


def test_null_arguments_and_unknown_ops():
    from ace_amd._lib import LIB, ACE_ERR_ARG
    assert LIB.ace_pl_host(None) == ACE_ERR_ARG and "NULL arguments" in LIB.ace_last_error().decode()
    for op in (-1, len(OPS)):
        rc, msg = _call(op, **_good("iterate"))
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


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name,value", [("batch", 0), ("batch", -3), ("m", 0), ("m", -1), ("d", 0), ("d", -2),
                                        ("guard", -1)])
def test_bad_sizes_are_argument_errors(op, name, value):
    from ace_amd._lib import ACE_ERR_ARG
    rc, msg = _call(op, **{**_good(op), name: value})
    assert rc == ACE_ERR_ARG and name in msg and f"({op})" in msg, (rc, msg)


@pytest.mark.parametrize("op", OPS)
def test_orders_beyond_the_eigensolver_are_unsupported(op):
    from ace_amd._lib import ACE_ERR_ARG, ACE_ERR_UNSUPPORTED
    rc, msg = _call(op, **{**_good(op), "d": 1601})
    assert rc == ACE_ERR_UNSUPPORTED and "d = 1601" in msg
    # 1600 passes the size checks (and stops at a NULL operand: nothing is launched)
    good = _good(op)
    first = next(k for k, v in good.items() if isinstance(v, np.ndarray))
    rc, msg = _call(op, **{**{k: v for k, v in good.items() if k != first}, "d": 1600})
    assert rc == ACE_ERR_ARG and f"NULL {first}" in msg


def test_the_reduced_final_vector_needs_a_square_r():
    from ace_amd._lib import ACE_ERR_ARG
    good = _good("final_vec")
    rc, msg = _call("final_vec", **{**good, "reduced": 1, "m": 5})
    assert rc == ACE_ERR_ARG and "NULL R" in msg
    rc, msg = _call("final_vec", **{**good, "reduced": 1, "R": np.ones(64)})
    assert rc == ACE_ERR_ARG and "reduced needs m == d" in msg


def test_python_mirror_refuses_bad_shapes_before_the_call():
    import ace_amd
    from ace_amd import plstep
    assert ace_amd.plstep is plstep and not hasattr(ace_amd, "pl_host")
    z = np.zeros
    with pytest.raises(ValueError, match="unknown op"):
        plstep.pl_host("nope", batch=1, m=3, d=2)
    with pytest.raises(TypeError, match="unknown ace_pl_args field"):
        plstep.pl_host("iterate", batch=1, m=3, d=2, nonsense=z(3))
    for kw in (dict(x=z((2, 3, 3))),                    # x is not [b][d][d]
               dict(Ax=z((2, 4))),                      # Ax is not [b][m]
               dict(R=z((3, 2))),                       # R is not [d][m]
               dict(state=z((2, 5)))):
        with pytest.raises(ValueError, match="expected shape"):
            plstep.pl_host("iterate", batch=2, m=3, d=2, **kw)
    # the C checks reach Python as AceError with the argument's name
    with pytest.raises(ace_amd.AceError, match="NULL gAx"):
        plstep.pl_host("iterate", batch=2, m=3, d=2, x=z((2, 2, 2)), Ax=z((2, 3)))
    with pytest.raises(ace_amd.AceError, match="d = 2000"):
        plstep.pl_host("chol", batch=1, m=3, d=2000)
    s = plstep.state_array(3, L=[1, 2, 3], theta=np.inf, done=[0, 1, 0])
    assert s[:, 0].tolist() == [1, 2, 3] and np.isinf(s[:, plstep.STATE.index("theta")]).all()
    assert s[:, plstep.STATE.index("done")].tolist() == [0, 1, 0] and s.shape == (3, len(plstep.STATE))
