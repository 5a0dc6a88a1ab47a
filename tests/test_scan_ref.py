"""CPU tests of the beam scan's reference (tests/scan_ref.py): it agrees with naive triple loops written from
the formula, it rejects four plausible wrong models on every realisation, and every parity case of the GPU
suite satisfies the precondition under which top_idx can be compared exactly."""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import scan_ref as SR  # noqa: E402

TINY = [(2, 2, 3, 3, 2), (3, 3, 2, 2, 4), (2, 4, 4, 5, 3)]   # (batch, d0, d1, Q0, Q1)


def _inputs(shape, seed=0):
    batch, d0, d1, Q0, Q1 = shape
    rng = np.random.default_rng([seed, *shape])
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)   # noqa: E731
    return c(batch, d0 * d1), c(Q0, d0), c(Q1, d1), 0.3 * c(batch, Q1 * Q0)


def _naive(X, W0, F1, noise):
    """P[b][p Q0 + q] = |sum_i sum_j conj(W0[q][i]) x_b[i + d0 j] F1[p][j] + noise|^2 by loops, in longdouble."""
    (Q0, d0), (Q1, d1) = W0.shape, F1.shape
    P = np.zeros((X.shape[0], Q1 * Q0), SR.LD)
    for b in range(X.shape[0]):
        for p in range(Q1):
            for q in range(Q0):
                y = SR.CLD(noise[b, p * Q0 + q])
                for i in range(d0):
                    for j in range(d1):
                        y += SR.CLD(np.conj(W0[q, i])) * SR.CLD(X[b, i + d0 * j]) * SR.CLD(F1[p, j])
                P[b, p * Q0 + q] = y.real * y.real + y.imag * y.imag
    return P


@pytest.mark.parametrize("shape", TINY, ids=[str(s) for s in TINY])
def test_reference_against_naive_loops(shape):
    X, W0, F1, noise = _inputs(shape)
    K = 3
    ref = SR.exact(X, W0, F1, K, noise)
    P = _naive(X, W0, F1, noise)
    # two longdouble evaluations in different orders: far inside the f64 tolerance
    assert np.all(np.abs(P - ref["power"]).astype(np.float64) <= 1e-3 * ref["tol_power"])
    for b in range(shape[0]):
        order = sorted(range(P.shape[1]), key=lambda f: (-P[b, f], f))[:K]
        assert ref["top_idx"][b].tolist() == order
        assert np.array_equal(ref["top_pow"][b], ref["power"][b, order])
    assert np.all(np.abs(ref["total"] - P.sum(axis=1)).astype(np.float64) <= 1e-3 * ref["tol_total"])
    # the f64 restatement lies inside the tolerance
    q = SR.ratios(ref, power=SR.scan(X, W0, F1, noise))
    assert q["power"] <= 1.0, q


def test_exact_path_for_integer_beams_matches_integer_arithmetic():
    c = SR.tie_case()
    X, W0, F1, nz = c["X"], c["W0"], c["F1"], c["noise"]
    assert SR._gaussian_integers(W0) and SR._gaussian_integers(F1)
    y = np.einsum("qi,bij,pj->bpq", W0.conj(), SR._mat(X, 5, 3), F1).reshape(4, -1) + nz   # small integers: exact in f64
    P = (y.real ** 2 + y.imag ** 2)
    assert np.array_equal(c["ref"]["power"].astype(np.float64), P) and np.array_equal(c["ref"]["power"], P.astype(SR.LD))
    assert SR.gaps(c["ref"], c["K"]) == 0.0                       # (it does hold ties among its leaders)
    e = SR.tie_case(all_equal=True)["ref"]
    assert np.all(e["power"] == 1) and e["top_idx"].tolist() == [list(range(16))] * 4


@pytest.mark.parametrize("model", SR.MODELS)
@pytest.mark.parametrize("shape", TINY, ids=[str(s) for s in TINY])
def test_wrong_models_fall_outside_the_tolerance(shape, model):
    X, W0, F1, noise = _inputs(shape, seed=1)
    ref = SR.exact(X, W0, F1, 1, noise)
    bad = SR.scan(X, W0, F1, noise, model=model)
    err = np.abs(bad.astype(SR.LD) - ref["power"]).astype(np.float64)
    assert np.all((err / ref["tol_power"]).max(axis=1) > 1.0), model   # every realisation
    assert SR.ratios(ref, power=SR.scan(X, W0, F1, noise))["power"] <= 1.0


@pytest.mark.parametrize("kind", SR.KINDS)
@pytest.mark.parametrize("shape", SR.SHAPES, ids=["x".join(map(str, s)) for s in SR.SHAPES])
def test_parity_cases_have_separated_leaders(shape, kind):
    """The condition on the inputs under which equal indices can be demanded: among ranks 1 .. K + 1 of every
    realisation, with and without noise, consecutive reference powers differ by more than 1e-9 relative (the
    tolerance of a power is below 1e-10 of it at these leaders)."""
    c = SR.case(shape, kind)
    K = c["K"]
    for name in ("ref", "ref_noise"):
        ref = c[name]
        assert SR.gaps(ref, K) > 1e-9, (shape, kind, name, SR.gaps(ref, K))
        top = ref["top_pow"].astype(np.float64)
        tol = np.take_along_axis(ref["tol_power"], ref["top_idx"].astype(np.int64), axis=1)
        assert np.all(tol <= 1e-10 * top), (shape, kind, name, float((tol / top).max()))
