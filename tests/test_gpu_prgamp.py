"""GPU tests of the batched PR-GAMP (ace_prgamp_solve_*, csrc/ace_prgamp.hip).

Target: the numpy restatement of tests/prgamp_ref.py, run in long double.  status, counts and the trace (iterations and
passed iterations of every gampEst call) are compared exactly: tests/test_prgamp_ref.py asserts, for every realisation,
that each discrete decision has a margin above 64 x the distance between the f64 and the long-double run.  xhat must
lie within the larger of (m + N) u ||x|| (the classical bound of sums of that length) and 16 x the f64 spread of the
recursion at that realisation (the distance from the long-double run of the f64 run and of the f64 run on permuted
atoms; 16 covers the device's log / exp / sqrt and the MFMA accumulation order); info and vals relative, built the
same way (the two dB figures of info as the ratios they are the logarithms of: prgamp_ref.info_err says why).  xhat is
compared as it stands: the global phase of a try is fixed by its draws, which are shared.

Shapes (m, N, batch): (33, 130, 17) on a coherent and on a Gaussian dictionary (m and N off the 16 and 32 grids, a
second, partial work-group); (1, 5, 2); (16, 16, 16); (64, 48, 3) with a dense signal; (256, 4096, 2), the limit; each
at the kernel handle (gamp_nit 8, nit_em 0, max_try 1) and at gamp_nit 30, nit_em 2, max_try 2.  The full MyCPR set
(200, 50, 100) runs on (64, 48, 3) with 4 active entries: tests/prgamp_ref.py says why the dense signal cannot be the
converging case.

Worst err / bound per case (xhat / info / vals), measured on the MI355X (DESIGN.md §4i has the table); status, counts
and trace equal for every realisation of all 13 cases:
coherent-33x130 handle 0.055 / 0.029 / 0.075; coherent-33x130 short 0.085 / 0.151 / 0.074; gauss-33x130 handle 0.059
/ 0.027 / 0.051; gauss-33x130 short 0.081 / 0.101 / 0.093; 1x5 handle 0.043 / 0.062 / 0.117; 1x5 short 0.084 / 0.144
/ 0.018; 16x16 handle 0.119 / 0.062 / 0.596; 16x16 short 0.229 / 0.518 / 0.107; dense-64x48 handle 0.066 / 0.031 /
0.021; dense-64x48 short 0.074 / 0.097 / 0.055; limit-256x4096 handle 0.003 / 0.001 / 0.001; limit-256x4096 short
0.078 / 0.086 / 0.089; sparse-64x48 mycpr 0.111 / 0.076 / 0.044.
"""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import prgamp_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [f"{s}-{h}" for s, h in PR.CASES]


def _dev(gpu, *arrays):
    import torch
    return [torch.from_numpy(np.array(a)).to(gpu) for a in arrays]


def _np(res):
    """(xhat, info, counts, status as uint32, trace, vals) on the host."""
    h = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return (h(res.xhat), h(res.info), h(res.counts), h(res.status).view(np.uint32), h(res.trace), h(res.vals))


def _same(a, b):
    return all((p is None and q is None) or np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


def _run(gpu, c, Y=None, G=None, trace=True, **kw):
    from ace_amd import prgamp_batch
    D, Yd, Gd = _dev(gpu, c["D"], c["Y"] if Y is None else Y, c["G"] if G is None else G)
    return prgamp_batch(D, Yd, c["lam"], draws=Gd, trace=trace, **c["kw"], **kw)


def _rel(a, b):
    return PR._rel(a, b)


@pytest.mark.parametrize("name,horizon", PR.CASES, ids=IDS)
def test_parity_with_the_reference(gpu, name, horizon):
    c = PR.case(name, horizon)
    xhat, info, cnt, st, tr, vals = _np(_run(gpu, c))
    fig = []
    for b, r in enumerate(c["ref"]):
        assert st[b] == r["status"], (b, st[b], r["status"])
        assert cnt[b].tolist() == r["counts"].tolist(), (b, cnt[b].tolist(), r["counts"].tolist())
        assert tr[b].tolist() == r["trace"].tolist(), (b, tr[b].tolist(), r["trace"].tolist())
        bx, bi, bv = PR.bound(c, b)
        ex = PR._dist(xhat[b], r["xhat"])
        fig.append((ex / bx, PR.info_err(info[b], r["info"]) / bi, _rel(vals[b], r["vals"]) / bv))
    for k, what in enumerate(("xhat", "info", "vals")):
        print(f"{name} {horizon}: err / bound per realisation  {what} " + " ".join(f"{q[k]:.3f}" for q in fig))
    print(f"{name} {horizon}: worst err / bound  xhat {max(q[0] for q in fig):.3f}  info {max(q[1] for q in fig):.3f}  "
          f"vals {max(q[2] for q in fig):.3f}")
    assert max(max(q) for q in fig) <= 1.0, fig


def test_bit_identity_alone_at_an_offset_without_extras_and_on_the_host(gpu):
    """The outputs of realisation b at batch 17 equal, bit for bit, those of the same input alone (batch 1) and at
    another position; neither the optional outputs nor the host twin change them."""
    from ace_amd import prgamp_host
    c = PR.case("coherent-33x130", "short")
    full = _np(_run(gpu, c))
    for b in range(17):
        one = _np(_run(gpu, c, Y=c["Y"][b:b + 1], G=c["G"][b:b + 1]))
        assert _same(one, [a[b:b + 1] for a in full]), b
    sub = _np(_run(gpu, c, Y=c["Y"][5:], G=c["G"][5:]))
    assert _same(sub, [a[5:] for a in full])
    bare = _run(gpu, c, trace=False)
    assert bare.trace is None and bare.vals is None and _same(_np(bare)[:4], full[:4])
    h = prgamp_host(c["D"], c["Y"], c["lam"], draws=c["G"], trace=True, **c["kw"])
    assert _same((h.xhat, h.info, h.counts, h.status, h.trace, h.vals), full)


def test_degenerate_and_failed_inputs(gpu):
    """y = 0 and a y whose squared norm overflows: the reference raises (CAwgnEstimIn's assert on xvar0 = 0; estFin_best
    never assigned), ACE_ST_PRGAMP_FAILED and zeros.  A non-finite y: ACE_ST_EVAL_DEGENERATE and zeros.  The neighbours
    in the batch are bitwise untouched."""
    from ace_amd import ACE_ST_EVAL_DEGENERATE, ACE_ST_PRGAMP_FAILED
    c = PR.case("gauss-33x130", "short")
    Yh = np.array(c["Y"][:6])
    Yh[1, 7] = np.nan
    Yh[2, 32] = np.inf
    Yh[3] = 0
    Yh[4] = Yh[4] * 1e160
    res = _run(gpu, c, Y=Yh, G=c["G"][:6])
    xhat, info, cnt, st, tr, vals = _np(res)
    plain = _np(_run(gpu, c, Y=c["Y"][:6], G=c["G"][:6]))
    assert st[1] == st[2] == ACE_ST_EVAL_DEGENERATE and st[3] == st[4] == ACE_ST_PRGAMP_FAILED
    assert res.failed.cpu().numpy().tolist() == [False, False, False, True, True, False]
    assert res.degenerate.cpu().numpy().tolist() == [False, True, True, False, False, False]
    for b in (1, 2, 3, 4):
        assert not xhat[b].any() and not info[b].any() and not tr[b].any() and not vals[b].any()
        assert cnt[b].tolist() == [0, 0, 0, -1]
        ref = PR.prgamp(c["D"], Yh[b], c["lam"], c["G"][b], **c["kw"])
        assert ref["status"] == st[b] and ref["counts"].tolist() == cnt[b].tolist()
    for b in (0, 5):
        assert _same([a[b] for a in (xhat, info, cnt, st, tr, vals)], [a[b] for a in plain])


def test_generated_draws_equal_the_same_draws_passed_in(gpu):
    from ace_amd import prgamp_batch, prgamp_draws
    c = PR.case("gauss-33x130", "short")
    D, Y = _dev(gpu, c["D"], c["Y"])
    seed, T, N = 20240611, c["kw"]["max_try"], c["D"].shape[1]
    a = prgamp_batch(D, Y, c["lam"], seed=seed, first=3, trace=True, **c["kw"])
    G = prgamp_draws(seed, Y.shape[0], T, N, gpu, first=3)
    b = prgamp_batch(D, Y, c["lam"], draws=G, trace=True, **c["kw"])
    assert _same(_np(a), _np(b))
    # the generator follows the stated counter layout: the host twin agrees to the rounding of log / cos / sin
    from ace_amd.prgamp import prgamp_draws_host
    assert np.allclose(G.cpu().numpy(), prgamp_draws_host(seed, Y.shape[0], T, N, first=3), rtol=1e-12, atol=1e-14)
    # other draws, another answer (the draws are read)
    other = prgamp_batch(D, Y, c["lam"], seed=seed + 1, first=3, trace=True, **c["kw"])
    assert not np.array_equal(_np(other)[0], _np(a)[0])
