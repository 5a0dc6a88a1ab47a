"""The batched A-optimal row exchange on the GPU (csrc/ace_aopt.hip, ace_amd/design.py) against the numpy restatement
tests/aopt_ref.py.

The selection is a chain of discrete decisions, so a comparison is only meaningful where the reference's own margins
leave room for another summation order: every test first asserts, on the reference alone, that the two smallest
exchange values of every step are at least 1e-6 apart (relative) and that no minimum of an assigned row is within
1e-10 of the cutoff.  Then rowlist, iters, switches and status must equal the reference's exactly.

acrit and Minv are compared with the brute-force inv(X^H X + kdiag I) of the GPU's own final rows.  The unit of that
comparison is the restatement's own discrepancy from the brute-force inverse at the same shape (rounding: measured
3.6e-16 .. 2.0e-15 relative for Minv, 1.0e-16 .. 1.1e-15 for the trace, floored at eps = 2.2e-16), and the GPU is
allowed FACTOR = 32 times it for its other summation order (butterfly sums in the matrix-vector products, a
Gauss-Jordan start instead of LAPACK's LU).  Measured on an MI355X: the GPU's discrepancy is 0.6 .. 2.5 units
(Minv 3.9e-16 .. 2.6e-15, trace 1.4e-16 .. 1.5e-15; the largest ratio is the trace at kdiag = 0.1); the table is in
DESIGN.md §4j, and every case prints its own figures before it asserts.
"""
import numpy as np
import pytest

import aopt_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(16, 64, 8, 1), (16, 64, 24, 2), (16, 96, 40, 3), (64, 128, 16, 4), (64, 200, 80, 5)]   # n, P, M, seed
RAGGED = (15, 37, 5, 11)   # n no multiple of 4, P no multiple of 16; seed 11 meets the condition (gap 1.2e-3, 3 passes)
FACTOR = 32.0
EPS = float(np.finfo(np.float64).eps)


def make(n, P, M, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 4, (P, n))
    F = np.exp(1j * np.pi / 2 * k) / np.sqrt(n)
    return F, rng.integers(0, P, M)


def condition(ref):
    """The reference's margins leave room for another summation order."""
    assert min(ref.gaps) >= 1e-6, min(ref.gaps)
    assert not ref.cut_margin or min(ref.cut_margin) >= 1e-10, min(ref.cut_margin)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def check_against_brute(F, rows, acrit_end, Minv, ref, kdiag=1.0, tag=""):
    """acrit and Minv of the GPU against the brute-force inverse of its own rows, in units of the reference's own
    discrepancy (FACTOR of them allowed)."""
    Mb = R.brute_minv(F, rows, kdiag)
    tb = float(np.trace(Mb).real)
    Mref = R.brute_minv(F, ref.rowlist, kdiag)
    unit_m = max(rel(ref.Minv, Mref), EPS)
    unit_a = max(abs(ref.acrit[1] - np.trace(Mref).real) / tb, EPS)
    got_m, got_a = rel(Minv, Mb), abs(acrit_end - tb) / tb
    print(f"aopt {tag}: Minv rel {got_m:.2e} (reference {unit_m:.2e}, ratio {got_m / unit_m:.1f}); "
          f"acrit rel {got_a:.2e} (reference {unit_a:.2e}, ratio {got_a / unit_a:.1f})")
    assert got_m <= FACTOR * unit_m, (got_m, unit_m)
    assert got_a <= FACTOR * unit_a, (got_a, unit_a)
    assert np.abs(Minv - Minv.conj().T).max() == 0.0   # the tracked inverse stays exactly Hermitian


def run_host(F, M, init, **kw):
    from ace_amd import design
    return design.aopt_select_host(F, M, init, want_minv=True, **kw)


def parity(res, ref, d=0):
    M = ref.rowlist.size
    assert np.array_equal(res.rowlist[d, :M], ref.rowlist), (res.rowlist[d, :M], ref.rowlist)
    assert (res.rowlist[d, M:] == -1).all()
    assert (int(res.iters[d]), int(res.switches[d]), int(res.status[d])) == (ref.iters, ref.switches, ref.status)


@pytest.mark.parametrize("shape", SHAPES + [RAGGED])
def test_parity_with_the_restatement(gpu, shape):
    F, init = make(*shape)
    ref = R.aopt_select(F, shape[2], init)
    condition(ref)
    res = run_host(F, shape[2], init)
    parity(res, ref)
    # the start's trace: an n x n inverse by elimination, first-order bound n cond(M) eps (relative)
    X = F[init]
    cond = float(np.linalg.cond(X.conj().T @ X + np.eye(shape[0])))
    assert abs(res.acrit[0, 0] - ref.acrit[0]) <= shape[0] * cond * EPS * ref.acrit[0]
    check_against_brute(F, res.rowlist[0], res.acrit[0, 1], res.Minv[0], ref, tag=str(shape))


def test_kdiag_and_maxiter(gpu):
    F, init = make(16, 64, 24, 2)
    for kw in (dict(kdiag=0.1), dict(maxiter=1), dict(kdiag=0.1, maxiter=1)):
        ref = R.aopt_select(F, 24, init, **kw)
        condition(ref)
        res = run_host(F, 24, init, **kw)
        parity(res, ref)
        check_against_brute(F, res.rowlist[0], res.acrit[0, 1], res.Minv[0], ref, kdiag=kw.get("kdiag", 1.0), tag=str(kw))
    assert ref.iters == 1
    # kdiag on the start's other path (fewer rows than n: the nrows x nrows system)
    F, init = make(64, 128, 16, 4)
    ref = R.aopt_select(F, 16, init, kdiag=0.1)
    condition(ref)
    res = run_host(F, 16, init, kdiag=0.1)
    parity(res, ref)
    check_against_brute(F, res.rowlist[0], res.acrit[0, 1], res.Minv[0], ref, kdiag=0.1, tag="(64, 128, 16, 4) kdiag 0.1")


@pytest.mark.parametrize("shape", [(16, 64, 8, 1), (64, 200, 80, 5)])
def test_duplicated_candidates_go_to_the_smaller_index(gpu, shape):
    F, init = make(*shape)
    F = F.copy()
    F[40] = F[3]
    ref = R.aopt_select(F, shape[2], init)
    condition(ref)                      # (entries that tie with the minimum exactly do not count as the second one)
    assert 3 in ref.rowlist and 40 not in ref.rowlist
    res = run_host(F, shape[2], init)
    parity(res, ref)
    assert 3 in res.rowlist[0] and 40 not in res.rowlist[0]


def ragged_designs():
    """Ten designs with ragged row counts on one F, twice over two tile groups: (F, nrows [10], init [10][80], the five
    row counts, their start rows)."""
    F, _ = make(64, 200, 80, 5)
    rng = np.random.default_rng(77)
    Ms = [8, 24, 40, 16, 80]
    inits = [rng.integers(0, 200, M) for M in Ms]
    order = list(range(5)) + list(range(4, -1, -1))
    nrows = np.array([Ms[i] for i in order], np.int32)
    init = np.full((10, 80), 199, np.int32)            # the padding is never read as a start row
    for d, i in enumerate(order):
        init[d, :Ms[i]] = inits[i]
    return F, nrows, init, Ms, inits


def test_batch_invariance(gpu):
    """Designs with ragged row counts on one F, twice over two tile groups (ten designs), equal their single-design
    calls bit for bit, with and without Minv_out, and the restatement."""
    import torch
    from ace_amd import design
    F, nrows, init, Ms, inits = ragged_designs()
    Fd = torch.as_tensor(F, device=gpu)
    call = lambda nr, ini, mv: design.aopt_select_batch(Fd, torch.as_tensor(nr, device=gpu),   # noqa: E731
                                                        torch.as_tensor(ini, device=gpu), want_minv=mv)
    host = lambda r: [None if x is None else x.cpu().numpy() for x in   # noqa: E731
                      (r.rowlist, r.acrit, r.iters, r.switches, r.status, r.Minv)]
    full, lean = host(call(nrows, init, True)), host(call(nrows, init, False))
    assert lean[5] is None
    for a, b in zip(full[:5], lean[:5]):
        assert np.array_equal(a, b)
    for i, M in enumerate(Ms):
        ref = R.aopt_select(F, M, inits[i])
        condition(ref)
        one = host(call(np.array([M], np.int32), np.asarray(inits[i], np.int32)[None], True))
        assert np.array_equal(one[0][0], ref.rowlist) and (int(one[2][0]), int(one[3][0])) == (ref.iters, ref.switches)
        for d in (i, 9 - i):
            assert np.array_equal(full[0][d, :M], one[0][0]) and (full[0][d, M:] == -1).all()
            for q in (1, 2, 3, 4):
                assert np.array_equal(full[q][d], one[q][0]), (q, d)
            assert np.array_equal(full[5][d].view(np.float64), one[5][0].view(np.float64)), d


def test_train_rows_aopt(gpu):
    """realtrace.train_rows(rows="aopt") returns rows of the pool whose design beats random subsets; "first" and
    "randperm" are what they were."""
    from ace_amd import design, realtrace
    from ace_amd.engine import randperm
    F, _ = make(16, 96, 40, 3)
    cb = np.concatenate([F[:50], np.ones((8, 16)) / 4.0, F[50:]])      # the pool leaves out rows 50..57
    pool = np.concatenate([np.arange(50), np.arange(58, 104)])
    rows = realtrace.train_rows(pool, 40, 1, "aopt", seed=7, cb=cb)
    assert rows.shape == (40,) and rows.dtype == np.int64 and np.isin(rows, pool).all()
    ref = R.aopt_select(F, 40, design.start_rows(7, 1, 96, 40))
    condition(ref)
    assert np.array_equal(rows, pool[ref.rowlist])
    tr = float(np.trace(R.brute_minv(cb, rows)).real)
    rng = np.random.default_rng(0)
    rnd = np.mean([np.trace(R.brute_minv(F, rng.choice(96, 40, replace=False))).real for _ in range(50)])
    print(f"aopt design trace {tr:.4f}, mean of 50 random subsets {rnd:.4f}")
    assert tr < rnd
    assert realtrace.train_rows(pool, 40, 1, "first", seed=7, cb=cb).tolist() == pool[:40].tolist()
    assert np.array_equal(realtrace.train_rows(pool, 40, 1, "randperm", seed=7, cb=cb),
                          pool[randperm(7, 1, 96, 40).astype(np.int64)])
    assert realtrace.train_rows(np.array([1, 2, 4, 5, 7, 8, 9, 11, 12, 13]), 5, 3, "randperm", seed=77).tolist() == [9, 2, 13, 12, 5]
