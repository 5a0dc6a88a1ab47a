"""CPU tests of the stage test entry's C-ABI (ace_stage_host) and of its Python mirror (ace_amd.stages): the argument
checks, which run before any HIP call.  No compute calls -- there is no GPU here."""
import ctypes as C

import numpy as np
import pytest

_dp, _ip, _bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_ubyte)


def _good(op):
    """Sizes and non-NULL dummy arrays that pass the checks of ``op`` (never dereferenced past the index tables: every
    case below breaks one of them)."""
    m, mt, n, r, b = 6, 4, 5, 2, 2
    z = np.zeros(4096)
    rows = np.tile(np.arange(m, dtype=np.int32), (b, 1))
    mask = np.tile((np.arange(m) < mt).astype(np.uint8), (b, 1))
    idx = np.arange(3, dtype=np.int32)
    base = dict(batch=b, n=n, m=m, r=r)
    return {
        "init_r": dict(base, mu0=1e-3, X=z, P0=z, B=z),
        "ystep_r": dict(base, S=z, g=z, M=z, Y=z, B=z),
        "finalize_r": dict(base, nc=1, optX=z, optY=z, X=z, Y=z),
        "gram_rotate": dict(base, X=z),
        "quality": dict(base, count=3, A=z, X=z, B=z),
        "part_quality": dict(base, mt=mt, A=z, X=z, B=z, rows=rows),
        "keep_best": dict(base, q=z, qmax=z, X=z, Y=z),
        "finish": dict(base, mt=mt, q=z, X=z, Y=z, Xmax=z, Ymax=z, anorm=z, bnorm=z),
        "part_geinv": dict(base, mt=mt, G=z, rows=rows),
        "part_gfix": dict(base, mt=mt, G=z, geinv=z, g=z, rows=rows, mask=mask),
        "part_expand": dict(base, mt=mt, Y=z, rows=rows),
        "part_compact": dict(base, mt=mt, Y=z, rows=rows),
        "anorm": dict(base, A=z),
        "bnorm": dict(base, B=z),
        "gather_rows": dict(base, count=3, A=z, idx=idx, anorm=z),
        "gather_b": dict(base, count=3, B=z, idx=idx),
        "move_rows": dict(base, count=3, len=4, src=z, idx=idx),
        "move_bytes": dict(base, count=3, len=4, bsrc=z.astype(np.uint8), idx=idx),
        "put_col": dict(base, count=3, ld=4, col=1, isrc=idx, idx=idx),
        "flag_bits": dict(base, count=3, bsrc=z.astype(np.uint8)),
        "fill": dict(base, len=3),
    }[op]


def _call(op, **kw):
    from ace_amd._lib import LIB, StageArgs
    from ace_amd.stages import OPS
    a = StageArgs()
    a.op = OPS[op] if isinstance(op, str) else op
    keep = []
    for k, v in kw.items():
        if isinstance(v, np.ndarray):
            tp = {np.dtype(np.int32): _ip, np.dtype(np.uint8): _bp}.get(v.dtype, _dp)
            keep.append(v)
            v = v.ctypes.data_as(tp)
        setattr(a, k, v)
    rc = LIB.ace_stage_host(C.byref(a))
    return rc, LIB.ace_last_error().decode()


ALL_OPS = ["init_r", "ystep_r", "finalize_r", "gram_rotate", "quality", "part_quality", "keep_best", "finish",
           "part_geinv", "part_gfix", "part_expand", "part_compact", "anorm", "bnorm", "gather_rows", "gather_b",
           "move_rows", "move_bytes", "put_col", "flag_bits", "fill"]


def test_the_op_table_matches_the_header():
    from ace_amd.stages import OPS
    assert list(OPS) == ALL_OPS
    text = (__import__("pathlib").Path(__file__).resolve().parents[1] / "include" / "ace.h").read_text()
    enum = text[text.index("ACE_STAGE_INIT_R = 0"):text.index("ACE_STAGE_NOPS")]
    names = [t.strip().split(" ")[0] for t in enum.replace("\n", " ").split(",") if t.strip()]
    assert [n[len("ACE_STAGE_"):].lower() for n in names] == ALL_OPS


def test_null_arguments_and_unknown_ops():
    from ace_amd._lib import LIB, ACE_ERR_ARG
    assert LIB.ace_stage_host(None) == ACE_ERR_ARG and "NULL arguments" in LIB.ace_last_error().decode()
    for op in (-1, len(ALL_OPS)):
        rc, msg = _call(op)
        assert rc == ACE_ERR_ARG and "unknown op" in msg


@pytest.mark.parametrize("op", ALL_OPS)
def test_every_array_is_required_by_name(op):
    from ace_amd._lib import ACE_ERR_ARG
    good = _good(op)
    optional = {"put_col": {"idx"}}.get(op, set())
    for name, v in good.items():
        if not isinstance(v, np.ndarray) or name in optional:
            continue
        rc, msg = _call(op, **{k: x for k, x in good.items() if k != name})
        assert rc == ACE_ERR_ARG and f"NULL {name}" in msg and f"({op})" in msg, (name, rc, msg)


@pytest.mark.parametrize("op,name,value", [
    ("init_r", "batch", 0), ("init_r", "batch", 4097), ("init_r", "n", 0), ("init_r", "m", 4097), ("init_r", "r", 0),
    ("init_r", "mu0", 0.0), ("ystep_r", "m", 0), ("ystep_r", "r", -1), ("finalize_r", "nc", 0), ("finalize_r", "nc", 3),
    ("gram_rotate", "n", 0), ("gram_rotate", "batch", -2), ("quality", "count", -1), ("quality", "n", 4097),
    ("part_quality", "mt", 0), ("part_quality", "mt", 7), ("keep_best", "m", 0), ("finish", "mt", 7),
    ("part_geinv", "m", 0), ("part_gfix", "mt", 0), ("part_expand", "r", 0), ("anorm", "n", 0), ("bnorm", "batch", 0),
    ("gather_rows", "count", -1), ("gather_b", "count", 4097), ("move_rows", "len", 0), ("move_bytes", "len", -4),
    ("put_col", "ld", 0), ("put_col", "col", 4), ("put_col", "count", -1), ("flag_bits", "count", 7),
    ("fill", "len", 7), ("fill", "m", 0)])
def test_bad_sizes_are_argument_errors(op, name, value):
    from ace_amd._lib import ACE_ERR_ARG
    rc, msg = _call(op, **{**_good(op), name: value})
    assert rc == ACE_ERR_ARG and name in msg, (rc, msg)


@pytest.mark.parametrize("op", ["init_r", "ystep_r", "finalize_r", "gram_rotate", "part_gfix", "part_expand",
                                "part_compact"])
def test_more_than_32_columns_is_unsupported(op):
    from ace_amd._lib import ACE_ERR_UNSUPPORTED
    rc, msg = _call(op, **{**_good(op), "r": 33})
    assert rc == ACE_ERR_UNSUPPORTED and "r = 33" in msg


@pytest.mark.parametrize("op", ["part_quality", "part_geinv", "part_gfix", "part_expand", "part_compact"])
def test_more_than_96_test_rows_is_unsupported(op):
    from ace_amd._lib import ACE_ERR_ARG, ACE_ERR_UNSUPPORTED
    m = 200
    rows = np.tile(np.arange(m, dtype=np.int32), (2, 1))
    rc, msg = _call(op, **{**_good(op), "m": m, "mt": m - 97, "rows": rows})
    assert rc == ACE_ERR_UNSUPPORTED and "m - mt = 97" in msg
    # 96 passes the size check (and stops at the NULL operand: nothing is launched)
    rc, msg = _call(op, **{**_good(op), "m": m, "mt": m - 96, "rows": rows[:, ::-1].copy(), "G": None, "A": None,
                           "Y": None})
    assert rc == ACE_ERR_ARG and "NULL" in msg and "m - mt" not in msg


def test_index_tables_are_checked_before_any_launch():
    from ace_amd._lib import ACE_ERR_ARG
    for op in ("part_quality", "part_geinv", "part_gfix", "part_expand", "part_compact"):
        for bad in (6, -1, 0):                                     # out of range twice, then a repeated row
            good = _good(op)
            rows = good["rows"].copy()
            rows[1, 3] = bad
            rc, msg = _call(op, **{**good, "rows": rows})
            assert rc == ACE_ERR_ARG and "rows" in msg, (op, bad, msg)
    good = _good("part_gfix")
    mask = good["mask"].copy()
    mask[0, 5] = 1                                                 # a test row marked as a train row
    rc, msg = _call("part_gfix", **{**good, "mask": mask})
    assert rc == ACE_ERR_ARG and "mask" in msg
    for op, lim in (("gather_rows", 6), ("gather_b", 6), ("move_rows", 6), ("move_bytes", 6), ("put_col", 6)):
        for bad in (lim, -1):
            good = _good(op)
            idx = good["idx"].copy()
            idx[2] = bad
            rc, msg = _call(op, **{**good, "idx": idx})
            assert rc == ACE_ERR_ARG and "idx" in msg, (op, bad, msg)
    for op in ("move_rows", "move_bytes", "put_col"):              # a scatter's destinations are distinct
        good = _good(op)
        idx = good["idx"].copy()
        idx[2] = idx[0]
        rc, msg = _call(op, **{**good, "idx": idx, "scatter": 1})
        assert rc == ACE_ERR_ARG and "idx" in msg, (op, msg)


def test_python_mirror_refuses_bad_shapes_before_the_call():
    import ace_amd
    from ace_amd import stages
    assert ace_amd.stages is stages and not hasattr(ace_amd, "stage_host")
    z = np.zeros
    with pytest.raises(ValueError, match="unknown op"):
        stages.stage_host("nope")
    with pytest.raises(TypeError, match="unknown ace_stage_args field"):
        stages.stage_host("fill", len=1, m=2, nonsense=np.zeros(3))
    with pytest.raises(ValueError, match="missing size"):
        stages.stage_host("gram_rotate", batch=1, n=4, X=z((1, 2, 4)))
    for kw in (dict(batch=2, n=4, r=2, X=z((2, 2, 5))),            # X is not [b][r][n]
               dict(batch=2, n=4, r=33, X=z((2, 33, 4))),           # r > 32
               dict(batch=2, n=4, r=2, X=z((2, 2, 4)), idst=z(3))):
        with pytest.raises(ValueError):
            stages.stage_host("gram_rotate", **kw)
    rows = np.tile(np.arange(200, dtype=np.int32), (1, 1))
    with pytest.raises(ValueError, match="test rows"):
        stages.stage_host("part_geinv", batch=1, m=200, mt=103, G=z((200, 200)), rows=rows)
    with pytest.raises(ValueError):
        stages.stage_host("part_gfix", batch=1, m=6, mt=4, r=1, G=z((6, 6)), geinv=z((1, 3, 3)), g=z((1, 1, 6)),
                          rows=rows[:, :6], mask=z((1, 6)))
    with pytest.raises(ValueError):
        stages.stage_host("ystep_r", batch=1, m=6, r=2, S=z((1, 2, 6)), g=z((1, 2, 6)), M=z((1, 2, 6)), Y=z((1, 2, 6)),
                          B=z((1, 6)), state=z((1, 3)))
    # the C checks reach Python as AceError with the argument's name
    with pytest.raises(ace_amd.AceError, match="NULL X"):
        stages.stage_host("gram_rotate", batch=1, n=4, r=2)
    s, f = stages.state_array(3, mu=[1, 2, 3], nB=0.5), stages.flags_array(3, done=[0, 1, 0])
    assert s[:, 0].tolist() == [1, 2, 3] and (s[:, 3] == 0.5).all() and f[:, 1].tolist() == [0, 1, 0]
    assert s.shape == (3, len(stages.STATE)) and f.shape == (3, len(stages.FLAGS)) and f.dtype == np.int32
