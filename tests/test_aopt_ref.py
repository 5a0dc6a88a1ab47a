"""The numpy restatement of the Bayesian A-optimal row exchange (tests/aopt_ref.py) against first principles: its
tracked criterion is the brute-force trace of the rows it selected, the criterion does not increase once every row is
assigned, maxiter is honoured and a duplicated candidate is picked at its smaller index.  No GPU."""
import numpy as np
import pytest

import aopt_ref as R

SHAPES = [(16, 64, 8, 1), (16, 64, 24, 2), (16, 96, 40, 3), (64, 128, 16, 4), (64, 200, 80, 5)]   # n, P, M, seed


def make(n, P, M, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 4, (P, n))
    F = np.exp(1j * np.pi / 2 * k) / np.sqrt(n)
    return F, rng.integers(0, P, M)


@pytest.fixture(scope="module")
def runs():
    out = {}
    for s in SHAPES:
        F, init = make(*s)
        out[s] = ((F, init), R.aopt_select(F, s[2], init))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_tracked_acrit_is_the_brute_force_trace(runs, shape):
    (F, init), r = runs[shape]
    assert r.status == 0 and r.rowlist.min() >= 0 and r.rowlist.max() < F.shape[0]
    Mb = R.brute_minv(F, r.rowlist)
    assert abs(r.acrit[1] - np.trace(Mb).real) <= 1e-12
    assert abs(r.acrit[0] - np.trace(R.brute_minv(F, init)).real) <= 1e-12
    assert np.abs(r.Minv - Mb).max() <= 1e-13 * np.abs(Mb).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_acrit_never_increases_after_pass_one(runs, shape):
    _, r = runs[shape]
    assert len(r.acrit_pass) == r.iters >= 2
    assert all(b <= a for a, b in zip(r.acrit_pass[1:], r.acrit_pass[2:]))
    assert r.acrit_pass[-1] <= r.acrit_pass[0]
    # the last pass of a run that ended before maxiter switched nothing
    if r.iters < 5:
        assert r.acrit_pass[-1] == r.acrit_pass[-2]


def test_the_margins_the_issue_quotes(runs):
    gaps = [min(runs[s][1].gaps) for s in SHAPES]
    assert np.allclose(gaps, [0.14, 0.020, 5.1e-4, 7.5e-3, 2.1e-4], rtol=0.05)
    assert [runs[s][1].iters for s in SHAPES] == [3, 5, 5, 4, 4]
    assert all(abs(min(runs[s][1].cut_margin) - 1.49e-8) < 1e-10 for s in SHAPES)


def test_maxiter_one_stops_after_one_pass():
    F, init = make(16, 64, 24, 2)
    r = R.aopt_select(F, 24, init, maxiter=1)
    assert r.iters == 1 and r.switches == 24 and len(r.acrit_pass) == 1 and not r.cut_margin
    full = R.aopt_select(F, 24, init)
    assert full.iters > 1 and full.acrit[1] < r.acrit[1]


@pytest.mark.parametrize("shape", [(16, 64, 8, 1), (64, 200, 80, 5)])
def test_a_duplicated_candidate_is_picked_at_its_smaller_index(shape):
    F, init = make(*shape)
    F = F.copy()
    F[40] = F[3]
    r = R.aopt_select(F, shape[2], init)
    assert 3 in r.rowlist and 40 not in r.rowlist
    assert abs(r.acrit[1] - np.trace(R.brute_minv(F, r.rowlist)).real) <= 1e-12
