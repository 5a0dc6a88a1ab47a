"""GPU tests of the batched EM-BG-GAMP (ace_gamp_solve_*, csrc/ace_gamp.hip).

Target: the numpy restatement of tests/gamp_ref.py, run in long double (in f64 at the limit shape).  em_iters, the
trace (iterations and pass mask of every gampEst call) and the status are compared exactly: tests/test_gamp_ref.py
asserts, for every realisation, the conditions that make those decisions well defined.  xhat and params must lie
within the larger of (d + N) u ||x|| (the classical bound of sums of that length) and 16 x the f64 spread of the
recursion at that realisation (the distance from the long-double run of the f64 run and of the f64 run on permuted
atoms; 16 covers the device's log / exp and the MFMA accumulation order); params relative, the same way.

Shapes (d, N, batch): (33, 130, 17) on a coherent and on a Gaussian dictionary (d off the 16 and 32 grids, N off the
16 and 32 grids, a second, partial work-group), each also with max_em_iter = 0 (one cold GAMP call) and 2; (1, 5, 2);
(16, 16, 16); (256, 4096, 3), the limit.  Both option sets.

Measured on the MI355X (DESIGN.md §4g has the table): em_iters, trace and status are equal for every realisation of
all 18 parity cases; worst err / bound over them: xhat 0.106 (16x16), params 0.412 (16x16 cs); the limit shape sits
at 0.007 / 0.001.
"""
import ctypes as C
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import gamp_ref as GR  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [f"{s}-{o}-em{m}" for s, o, m in GR.CASES]


def _dev(gpu, *arrays):
    import torch
    return [torch.from_numpy(np.array(a)).to(gpu) for a in arrays]


def _np(res):
    """(xhat, params, em_iters, status as uint32, trace, xvar) on the host."""
    h = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return (h(res.xhat), h(res.params), h(res.em_iters), h(res.status).view(np.uint32), h(res.trace), h(res.xvar))


def _same(a, b):
    return all((p is None and q is None) or np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


def _run(gpu, c, Y=None, **kw):
    from ace_amd import embgamp_batch
    D, Yd = _dev(gpu, c["D"], c["Y"] if Y is None else Y)
    k = c["kw"]
    return embgamp_batch(D, Yd, c["snr"], c["lam"], learn_lambda=k["learn_lambda"], max_em_iter=k["max_em_iter"],
                         trace=True, want_xvar=True, **kw)


@pytest.mark.parametrize("name,optset,max_em", GR.CASES, ids=IDS)
def test_parity_with_the_reference(gpu, name, optset, max_em):
    c = GR.case(name, optset, max_em)
    xhat, par, emi, st, tr, xvar = _np(_run(gpu, c))
    fig = []
    for b, r in enumerate(c["ref"]):
        assert st[b] == r["status"], (b, st[b], r["status"])
        assert emi[b] == r["em_iters"], (b, emi[b], r["em_iters"])
        want = np.zeros((max_em + 1, 2), np.int64)
        want[:len(r["trace"])] = r["trace"]
        assert tr[b].tolist() == want.tolist(), (b, tr[b][:len(r["trace"]) + 1].tolist(), r["trace"])
        bx, bp = GR.bound(c, b)
        ex = float(np.sqrt(GR._abs2(xhat[b].astype(GR.CLD) - r["xhat"]).sum()))
        ep = float(np.max(np.abs((par[b].astype(GR.LD) - r["params"]) / r["params"])))
        fig.append((ex / bx, ep / bp))
        assert np.isfinite(xvar[b]).all()
    print(f"{name} {optset} max_em={max_em}: err / bound per realisation  xhat " + " ".join(f"{q:.3f}" for q, _ in fig)
          + "  params " + " ".join(f"{q:.3f}" for _, q in fig))
    print(f"{name} {optset} max_em={max_em}: worst err / bound  xhat {max(q for q, _ in fig):.3f}  "
          f"params {max(q for _, q in fig):.3f}")
    assert max(q for q, _ in fig) <= 1.0 and max(q for _, q in fig) <= 1.0, fig


def test_bit_identity_alone_at_an_offset_without_extras_and_on_the_host(gpu):
    """The outputs of realisation b at batch 17 equal, bit for bit, those of the same input alone (batch 1) and at
    another position; neither the optional outputs nor the host twin change them."""
    from ace_amd import embgamp_batch, embgamp_host
    c = GR.case("coherent-33x130", "plgamp", 200)
    full = _np(_run(gpu, c))
    assert len(set(full[2].tolist())) > 1   # (the realisations of a block stop at different EM iterations)
    for b in range(17):
        one = _np(_run(gpu, c, Y=c["Y"][b:b + 1]))
        assert _same(one, [a[b:b + 1] for a in full]), b
    sub = _np(_run(gpu, c, Y=c["Y"][5:]))
    assert _same(sub, [a[5:] for a in full])
    D, Y = _dev(gpu, c["D"], c["Y"])
    bare = embgamp_batch(D, Y, c["snr"], c["lam"])
    assert bare.trace is None and bare.xvar is None and _same(_np(bare)[:4], full[:4])
    h = embgamp_host(c["D"], c["Y"], c["snr"], c["lam"], trace=True, want_xvar=True)
    assert _same((h.xhat, h.params, h.em_iters, h.status, h.trace, h.xvar), full)


def test_degenerate_and_failed_inputs(gpu):
    """A non-finite y: ACE_ST_EVAL_DEGENERATE and zeros.  y = 0 and a y whose squared norm overflows: the reference's
    CAwgnEstimIn assert (initial phi 0 / NaN), ACE_ST_GAMP_FAILED and zeros.  The neighbours are untouched."""
    from ace_amd import ACE_ST_EVAL_DEGENERATE, ACE_ST_GAMP_FAILED
    c = GR.case("gauss-33x130", "plgamp", 200)
    Yh = np.array(c["Y"][:6])
    Yh[1, 7] = complex(np.nan, 0.0)
    Yh[2, 32] = complex(0.0, np.inf)
    Yh[3] = 0
    Yh[4] = Yh[4] * 1e160
    res = _run(gpu, c, Y=Yh)
    xhat, par, emi, st, tr, xvar = _np(res)
    plain = _np(_run(gpu, c, Y=c["Y"][:6]))
    assert st[1] == st[2] == ACE_ST_EVAL_DEGENERATE and st[3] == st[4] == ACE_ST_GAMP_FAILED
    assert res.failed.cpu().numpy().tolist() == [False, False, False, True, True, False]
    assert res.degenerate.cpu().numpy().tolist() == [False, True, True, False, False, False]
    for b in (1, 2, 3, 4):
        assert not xhat[b].any() and not xvar[b].any() and emi[b] == 0 and not tr[b].any()
        ref = GR.embgamp(c["D"], Yh[b], c["snr"], c["lam"])
        assert ref["status"] == st[b] and ref["em_iters"] == 0
    for b in (0, 5):
        assert _same([a[b] for a in (xhat, par, emi, st, tr, xvar)], [a[b] for a in plain])


def test_argument_errors_come_before_any_hip_call(gpu):
    from ace_amd._lib import LIB, gamp_cfg, ACE_ERR_ARG, ACE_ERR_UNSUPPORTED, ACE_ERR_WORKSPACE
    one = C.c_void_p(16)   # never dereferenced: the checks come first
    good = dict(snr_db=0.0, lambda0=0.1)

    def call(cfg=None, batch=3, d=5, N=7, xhat=one, ws=one, nbytes=1 << 30, **ck):
        cfg = gamp_cfg(**{**good, **ck}) if cfg is None else cfg
        return LIB.ace_gamp_solve_batch(C.byref(cfg), batch, d, N, one, one, xhat, None, one, one, None, None, ws, nbytes,
                                        None)

    assert call(d=257) == ACE_ERR_UNSUPPORTED and b"d 257" in LIB.ace_last_error()
    assert call(N=16385) == ACE_ERR_UNSUPPORTED
    assert call(d=0) == ACE_ERR_ARG and call(N=0) == ACE_ERR_ARG and call(batch=0) == ACE_ERR_ARG
    assert call(lambda0=0.0) == ACE_ERR_ARG and b"lambda0" in LIB.ace_last_error()
    assert call(lambda0=1.5) == ACE_ERR_ARG and call(lambda0=float("nan")) == ACE_ERR_ARG
    assert call(snr_db=float("inf")) == ACE_ERR_ARG
    assert call(max_em_iter=-1) == ACE_ERR_ARG and b"max_em_iter" in LIB.ace_last_error()
    assert call(gamp_nit=0) == ACE_ERR_ARG and call(gamp_nit=32) == ACE_ERR_ARG
    assert call(step0=0.0) == ACE_ERR_ARG and call(step0=1.5) == ACE_ERR_ARG and call(gamp_tol=-1.0) == ACE_ERR_ARG
    assert call(xhat=None) == ACE_ERR_ARG and b"NULL xhat" in LIB.ace_last_error()
    assert call(ws=None) == ACE_ERR_WORKSPACE
    need = int(LIB.ace_gamp_workspace_size(3, 5, 7))
    assert call(nbytes=need - 1) == ACE_ERR_WORKSPACE and b"workspace" in LIB.ace_last_error()
    assert LIB.ace_gamp_solve_batch(None, 3, 5, 7, one, one, one, None, one, one, None, None, one, 1 << 30, None) == ACE_ERR_ARG
