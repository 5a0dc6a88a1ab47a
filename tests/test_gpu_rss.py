"""GPU tests of the held-out RSS evaluator (ace_rss_evaluate_*: Evaluate_rss.m on the device, csrc/ace_rsseval.hip).

Target: the exact reference of tests/rss_ref.py (products without rounding, modulus and statistics in
longdouble) inside the tolerance derived there from the kernel's own accumulation: per entry of pred
4 (2n + 4) u sum_k |CB[p][k]| |X[b][k]|, propagated through / rss_p and the Pt-term sums for mean, rms and max.
n_used, the status word and the values of degenerate realisations are compared exactly.

The kernel's work-group takes 16 realisations and walks all the test rows in tiles of 128, so the shapes cover:
the K-loop tail (n = 1, 9: not a multiple of the 16-wide step; 144 / 16 = 9 steps), masked realisation and row
tiles (batch 3, 5, 17, 33; Pt 1, 5, 33, 70), a single full tile (16, 256, 16), several row tiles in one
work-group (Pt = 257: 3, Pt = 1200: 10, the last one masked) and several work-groups (batch 17, 33, 64: 2, 3, 4).
The test rows are never spread over work-groups, so there is no cross-group pass to exercise.

Worst err / tol measured on the MI355X over all parity cases and the skip case: pred 0.055, mean 0.056, rms 0.028,
max 0.057, all at (1, 1, 1); from n = 64 on pred stays below 0.005 and the statistics below 0.001.
"""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import rss_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(s, k) for s in RR.SHAPES for k in RR.KINDS]
IDS = [f"{b}x{n}x{p}-{k}" for (b, n, p), k in CASES]


def _dev(gpu, *arrays):
    import torch
    return [torch.from_numpy(np.array(a)).to(gpu) for a in arrays]   # (a copy: the shared inputs are read-only)


def _np(res):
    """(metrics, status as uint32, pred or None) of a device RssEval on the host."""
    pred = None if res.pred is None else res.pred.cpu().numpy()
    return res.metrics.cpu().numpy(), res.status.cpu().numpy().view(np.uint32), pred


def _compare(met, st, pred, ref, what):
    assert np.array_equal(st, ref["status"]), (what, st, ref["status"])
    assert np.array_equal(met[:, 3], ref["metrics"][:, 3].astype(np.float64)), what
    q = RR.ratios(met, pred, ref)
    print(f"{what}: worst err/tol " + " ".join(f"{k} {v:.3f}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, (what, q)
    return q


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_parity_with_the_exact_reference(gpu, shape, kind):
    from ace_amd import evaluate_rss_batch, evaluate_rss_host
    c = RR.case(*shape, kind)
    X, CB, rss = _dev(gpu, c["X"], c["CB"], c["rss"])
    res = evaluate_rss_batch(X, CB, rss, want_pred=True)
    met, st, pred = _np(res)
    assert (st == 0).all() and np.isfinite(met).all() and np.isfinite(pred).all()
    _compare(met, st, pred, c["ref"], f"{shape} {kind}")
    for i, name in enumerate(("mean_rel", "rms_rel", "max_rel", "n_used")):
        assert np.array_equal(getattr(res, name).cpu().numpy(), met[:, i])
    # the host entry runs the same kernel on copies: the same bits
    hres = evaluate_rss_host(c["X"], c["CB"], c["rss"], want_pred=True)
    assert np.array_equal(hres.metrics, met) and np.array_equal(hres.pred, pred) and np.array_equal(hres.status, st)


def test_bit_identity_alone_without_pred_shared_rss_and_on_a_stream(gpu):
    """A realisation's numbers are a function of (X_b, CB, rss_b, n, Pt) alone."""
    import torch
    from ace_amd import evaluate_rss_batch
    c = RR.case(33, 144, 257, "random")
    X, CB, rss = _dev(gpu, c["X"], c["CB"], c["rss"])
    full = evaluate_rss_batch(X, CB, rss, want_pred=True)
    met, st, pred = _np(full)
    # each realisation alone: batch 1, b = 0
    for b in range(33):
        one = evaluate_rss_batch(X[b:b + 1], CB, rss[b:b + 1], want_pred=True)
        m1, s1, p1 = _np(one)
        assert np.array_equal(m1[0], met[b]) and s1[0] == st[b] and np.array_equal(p1[0], pred[b]), b
    # a sub-batch at another offset (realisation 20 becomes row 0 of a 13-batch)
    m2, s2, p2 = _np(evaluate_rss_batch(X[20:], CB, rss[20:], want_pred=True))
    assert np.array_equal(m2, met[20:]) and np.array_equal(p2, pred[20:]) and np.array_equal(s2, st[20:])
    # without pred
    nop = evaluate_rss_batch(X, CB, rss)
    assert nop.pred is None
    m3, s3, _ = _np(nop)
    assert np.array_equal(m3, met) and np.array_equal(s3, st)
    # rss_shared = 1 against the same rss replicated
    r0 = rss[7].contiguous()
    ms, ss, ps = _np(evaluate_rss_batch(X, CB, r0, want_pred=True))
    mr, sr, pr = _np(evaluate_rss_batch(X, CB, r0[None].repeat(33, 1), want_pred=True))
    assert np.array_equal(ms, mr) and np.array_equal(ss, sr) and np.array_equal(ps, pr)
    assert np.array_equal(ps, pred)   # (pred does not depend on rss)
    # a non-default stream, and out= reuse
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        on_s = evaluate_rss_batch(X, CB, rss, want_pred=True)
    explicit = evaluate_rss_batch(X, CB, rss, want_pred=True, stream=s)
    s.synchronize()
    for r in (on_s, explicit):
        m4, s4, p4 = _np(r)
        assert np.array_equal(m4, met) and np.array_equal(s4, st) and np.array_equal(p4, pred)
    full.metrics.fill_(-1.0)
    again = evaluate_rss_batch(X, CB, rss, want_pred=True, out=full)
    assert again.metrics.data_ptr() == full.metrics.data_ptr() and again.pred.data_ptr() == full.pred.data_ptr()
    assert np.array_equal(again.metrics.cpu().numpy(), met)
    with pytest.raises(ValueError):
        evaluate_rss_batch(X[:5], CB, rss[:5], out=full)
    with pytest.raises(ValueError):
        evaluate_rss_batch(X, CB, rss, want_pred=True, out=nop)


def test_skip_and_degenerate_rules(gpu):
    from ace_amd import evaluate_rss_batch
    c = RR.skip_case()
    ref = c["ref"]
    X, CB, rss, Xp, rssp = _dev(gpu, c["X"], c["CB"], c["rss"], c["plain"]["X"], c["plain"]["rss"])
    res = evaluate_rss_batch(X, CB, rss, want_pred=True)
    met, st, pred = _np(res)
    assert sorted(np.nonzero(st & RR.ST_DEGENERATE)[0]) == c["degenerate"]
    assert sorted(np.nonzero(st & RR.ST_SKIPPED)[0]) == c["skipped"]
    assert (st & ~np.uint32(RR.ST_DEGENERATE | RR.ST_SKIPPED) == 0).all()
    assert np.array_equal(res.degenerate.cpu().numpy(), (st & RR.ST_DEGENERATE) != 0)
    assert np.array_equal(res.skipped.cpu().numpy(), (st & RR.ST_SKIPPED) != 0)
    for b in c["degenerate"]:
        assert np.array_equal(met[b], [1.0, 1.0, 1.0, 0.0]), (b, met[b])
    # an all-zero X: exactly 1, 1, 1, n_used = Pt, pred = 0 and no flag
    z = c["zero"]
    assert np.array_equal(met[z], [1.0, 1.0, 1.0, 33.0]) and st[z] == 0 and not pred[z].any()
    fin = [b for b in range(12) if b not in (7, 8)]
    _compare(met[fin], st[fin], pred[fin], {k: v[fin] for k, v in ref.items()}, "skip case")
    assert np.array_equal(met[[7, 8], 3], [0.0, 0.0]) and not np.isfinite(pred[[7, 8]]).any()
    # pred is still written for skipped rows, and is what the plain inputs give there; the neighbours of the
    # special realisations are unaffected bit for bit
    mp, sp, pp = _np(evaluate_rss_batch(Xp, CB, rssp, want_pred=True))
    assert (sp == 0).all()
    for b in c["plain_rows"]:
        assert np.array_equal(met[b], mp[b]) and np.array_equal(pred[b], pp[b])
    for b in (1, 2, 3, 4, 5, 6):
        assert np.array_equal(pred[b], pp[b]), b


def test_guard_regions(gpu):
    """X, CB, rss, metrics and pred inside larger NaN-filled tensors at (17, 64, 33): the same results, and the
    guards of the outputs untouched (a read past an input's end would bring a NaN in; accesses past the end are
    bugs even where the values are discarded)."""
    import torch
    from ace_amd import RssEval, evaluate_rss_batch
    c = RR.case(17, 64, 33, "random")
    X, CB, rss = _dev(gpu, c["X"], c["CB"], c["rss"])
    met, st, pred = _np(evaluate_rss_batch(X, CB, rss, want_pred=True))
    G = 64   # guard elements on each side

    def guarded(t):
        real = torch.view_as_real(t) if t.is_complex() else t
        buf = torch.full((real.numel() + 2 * G,), float("nan"), dtype=torch.float64, device=gpu)
        buf[G:G + real.numel()] = real.reshape(-1)
        inner = buf[G:G + real.numel()].view(real.shape)
        return buf, (torch.view_as_complex(inner) if t.is_complex() else inner)

    _, Xg = guarded(X)
    _, CBg = guarded(CB)
    _, rg = guarded(rss)
    mbuf, mg = guarded(torch.zeros((17, 4), dtype=torch.float64, device=gpu))
    pbuf, pg = guarded(torch.zeros((17, 33), dtype=torch.float64, device=gpu))
    sg = torch.full((17 + 2 * G,), -7, dtype=torch.int32, device=gpu)
    out = RssEval(mg[:, 0], mg[:, 1], mg[:, 2], mg[:, 3], sg[G:G + 17], mg, pg)
    res = evaluate_rss_batch(Xg, CBg, rg, want_pred=True, out=out)
    assert res.metrics.data_ptr() == mg.data_ptr() and res.pred.data_ptr() == pg.data_ptr()
    m2, s2, p2 = _np(res)
    assert np.array_equal(m2, met) and np.array_equal(s2, st) and np.array_equal(p2, pred)
    for buf, nel in ((mbuf, 17 * 4), (pbuf, 17 * 33)):
        assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + nel:]).all()
    assert (sg[:G] == -7).all() and (sg[G + 17:] == -7).all()
    # the shared-rss form reads one row only: a [Pt] vector with guards
    _, r1 = guarded(rss[0].contiguous())
    m3, _, _ = _np(evaluate_rss_batch(Xg, CBg, r1))
    assert np.array_equal(m3[0], met[0])
