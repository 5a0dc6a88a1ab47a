"""CPU tests of the held-out RSS references (tests/rss_ref.py) and of the pure helpers of ace_amd.realtrace: the
f64 restatement against the exact version inside the derived tolerance, four deliberately wrong models outside
it, the tracker's probe-budget rule and the sweep's row split.  No GPU.

Worst err / tol of the f64 restatement against the exact reference over the GPU suite's inputs (both codebook
kinds, the skip case included): pred 0.055, mean 0.056, rms 0.028, max 0.057 (all at n = 1, where the bound
has the least slack; from n = 64 on every ratio is below 0.005)."""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import rss_ref as RR  # noqa: E402

CASES = [(s, k) for s in RR.SHAPES for k in RR.KINDS]
IDS = [f"{b}x{n}x{p}-{k}" for (b, n, p), k in CASES]


def _check_exact_fields(met, st, ref):
    assert np.array_equal(st, ref["status"])
    assert np.array_equal(met[:, 3], ref["metrics"][:, 3].astype(np.float64))
    dg = (ref["status"] & RR.ST_DEGENERATE) != 0
    assert np.array_equal(met[dg], np.tile([1.0, 1.0, 1.0, 0.0], (int(dg.sum()), 1)))


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_f64_restatement_is_inside_the_derived_tolerance(shape, kind):
    c = RR.case(*shape, kind)
    met, st, pred = RR.evaluate_rss(c["X"], c["CB"], c["rss"])
    _check_exact_fields(met, st, c["ref"])
    q = RR.ratios(met, pred, c["ref"])
    print(shape, kind, q)
    assert max(q.values()) <= 1.0, q


def test_f64_restatement_on_the_skip_case():
    c = RR.skip_case()
    met, st, pred = RR.evaluate_rss(c["X"], c["CB"], c["rss"])
    ref = c["ref"]
    _check_exact_fields(met, st, ref)
    fin = [b for b in range(12) if b not in (7, 8)]
    q = RR.ratios(met[fin], pred[fin], {k: v[fin] for k, v in ref.items()})
    print(q)
    assert max(q.values()) <= 1.0, q
    assert sorted(np.nonzero(st & RR.ST_DEGENERATE)[0]) == c["degenerate"]
    assert sorted(np.nonzero(st & RR.ST_SKIPPED)[0]) == c["skipped"]
    assert np.array_equal(met[c["zero"]], [1.0, 1.0, 1.0, 33.0]) and st[c["zero"]] == 0
    assert met[5, 3] == 29 and met[1, 3] == 31


# (at n = 1 the conjugate has the same modulus, |conj(c) x| = |c x|: the conjugated model is not wrong there)
WRONG = [(m, s, k) for m in ("conj", "square", "diff_first") for s, k in CASES if not (m == "conj" and s[1] == 1)]


@pytest.mark.parametrize("model,shape,kind", WRONG, ids=[f"{m}-{b}x{n}x{p}-{k}" for m, (b, n, p), k in WRONG])
def test_wrong_models_land_outside_the_tolerance(model, shape, kind):
    """A conjugated CB, |.|^2 in place of |.| and the difference taken before the modulus: every realisation's
    mean_rel misses the exact value by more than the tolerance."""
    c = RR.case(*shape, kind)
    met, _, _ = RR.evaluate_rss(c["X"], c["CB"], c["rss"], model=model)
    ref = c["ref"]
    err = np.abs(met[:, 0].astype(np.longdouble) - ref["metrics"][:, 0]).astype(np.float64)
    assert (err > ref["tol"][:, 0]).all(), (err / ref["tol"][:, 0]).min()


def test_dividing_by_pt_lands_outside_the_tolerance_when_rows_are_skipped():
    c = RR.skip_case()
    met, st, _ = RR.evaluate_rss(c["X"], c["CB"], c["rss"], model="div_pt")
    ref = c["ref"]
    rows = [b for b in c["skipped"] if b not in c["degenerate"]]
    for col in (0, 1):
        err = np.abs(met[rows, col].astype(np.longdouble) - ref["metrics"][rows, col]).astype(np.float64)
        assert (err > ref["tol"][rows, col]).all()


# ---------------------------------------------------------------- realtrace's pure helpers
NEXT_M = [  # (M, err, m_max, threshold, expected)
    (80, 0.1, 80, 0.2, 63), (80, 0.3, 80, 0.2, 80), (63, 0.1, 80, 0.2, 50), (63, 0.3, 80, 0.2, 76),
    (76, 0.9, 80, 0.2, 80), (4, 0.0, 80, 0.2, 3), (3, 0.0, 80, 0.2, 2), (1, 0.0, 80, 0.2, 0),
    (0, 0.0, 80, 0.2, 0), (0, 0.5, 80, 0.2, 1), (1, 0.5, 80, 0.2, 2), (5, 0.5, 80, 0.2, 7),
    (10, 0.2, 80, 0.2, 13),              # err == threshold is not below it
    (10, 0.19999, 80, 0.2, 7), (20, 1.0, 24, 0.2, 24), (24, 1.0, 24, 0.2, 24),
    (24, 5.0, 24, float("inf"), 19), (10, float("nan"), 80, 0.2, 13),   # a NaN score is not below the threshold
]


@pytest.mark.parametrize("M,err,m_max,thr,want", NEXT_M)
def test_next_m(M, err, m_max, thr, want):
    from ace_amd.realtrace import next_m
    assert next_m(M, err, m_max, thr) == want


def test_next_m_walks_down_to_zero_and_back_up_to_the_cap():
    from ace_amd.realtrace import next_m
    M, seq = 80, []
    while M:
        seq.append(M)
        M = next_m(M, 0.0, 80, 0.2)
    assert seq == [80, 63, 50, 39, 31, 24, 19, 15, 11, 8, 6, 4, 3, 2, 1]
    up = [0]
    while up[-1] < 80:
        up.append(next_m(up[-1], 1.0, 80, 0.2))
    assert up == [0, 1, 2, 3, 4, 5, 7, 9, 11, 14, 17, 21, 26, 32, 39, 47, 57, 69, 80]


def test_split_rows():
    from ace_amd.realtrace import split_rows
    pool, test = split_rows(10, n_test=3)
    assert pool.tolist() == [0, 1, 2, 3, 4, 5, 6] and test.tolist() == [7, 8, 9]
    pool, test = split_rows(8, test_rows=[5, 0, 3])
    assert pool.tolist() == [1, 2, 4, 6, 7] and test.tolist() == [5, 0, 3]   # the test rows keep their given order
    for kw in ({}, {"n_test": 2, "test_rows": [1]}, {"n_test": 0}, {"n_test": 8}, {"test_rows": [8]},
               {"test_rows": [-1]}, {"test_rows": [1, 1]}, {"test_rows": []}, {"test_rows": list(range(8))}):
        with pytest.raises(ValueError):
            split_rows(8, **kw)


def test_train_rows():
    from ace_amd import engine
    from ace_amd.realtrace import train_rows
    pool = np.array([1, 2, 4, 6, 7, 9, 11, 12])
    assert train_rows(pool, 3, 0).tolist() == [1, 2, 4]
    assert train_rows(pool, 8, 5, "first").tolist() == pool.tolist()
    for k in (0, 3):
        got = train_rows(pool, 5, k, "randperm", seed=77)
        assert got.tolist() == pool[engine.randperm(77, k, 8, 5)].tolist()
        assert len(set(got.tolist())) == 5 and set(got.tolist()) <= set(pool.tolist())
    assert train_rows(pool, 5, 0, "randperm", seed=77).tolist() != train_rows(pool, 5, 1, "randperm", seed=77).tolist()
    for bad in ((0, "first"), (9, "first"), (3, "last")):
        with pytest.raises(ValueError):
            train_rows(pool, bad[0], 0, bad[1])
