"""CPU tests (numpy only) of the host side of the sparse recoveries (ace_amd/sparse.py): the two-stage compression
rule of My_TwoStage_Recovery.m:78-100, the 2-D angular dictionary of Sparse_Channel_Formulation.m:136-143, and the
coherent measurement the PerfectPhaseCS benchmark runs on."""
import math

import numpy as np
import pytest

from ace_amd import angular, sparse, synth


def _phase_code_beams(rng, M, n):
    return (1j ** rng.integers(0, 4, (M, n))) / np.sqrt(n)


def _rule(dS, m, n, s):
    """An independent restatement of My_TwoStage_Recovery.m:79-94 on the singular values alone."""
    rnd = lambda x: int(np.floor(x + 0.5))   # noqa: E731  (MATLAB's round on positive numbers)
    mCS = min(rnd(1.75 * s * np.log(n / s)), len(dS)) - 1
    ratio = np.cumsum(dS) / np.sum(dS)
    while (ratio[mCS - 1] if mCS > 0 else 0.0) < 0.80 and mCS < len(dS):
        mCS += 1
    while rnd(1.75 * mCS * np.log(mCS)) < m and mCS < len(dS):
        mCS += 1
    return mCS


@pytest.fixture(scope="module")
def AD16():
    return sparse.dictionary_2d(16, 16)[0]


def test_two_stage_setup_dimensions_at_16x16(AD16):
    """mCS = 46, 135, 155, 175 at M = 64, 256, 400, 1024 for phase-code beams from default_rng(3) (they depend on the
    draw only through the 80 % rule), and P C is the rank-mCS truncation of Phi."""
    assert AD16.shape == (256, 2401)
    rng = np.random.default_rng(3)
    got = {}
    for M in (64, 256, 400, 1024):
        Phi = _phase_code_beams(rng, M, 256) @ AD16
        ts = sparse.two_stage_setup(Phi, 3)
        U, dS, Vh = np.linalg.svd(Phi, full_matrices=False)
        assert ts.mCS == _rule(dS, M, 2401, 3)
        got[M] = ts.mCS
        assert ts.P.shape == (M, ts.mCS) and ts.C.shape == (ts.mCS, 2401)
        trunc = (U[:, :ts.mCS] * dS[:ts.mCS]) @ Vh[:ts.mCS]
        assert np.linalg.norm(ts.P @ ts.C - trunc) <= 1e-12 * np.linalg.norm(trunc)
        # P and C split the singular values evenly: P^H P = C C^H = diag(S)
        assert np.allclose(ts.P.conj().T @ ts.P, np.diag(dS[:ts.mCS]), atol=1e-12 * dS[0])
        assert np.allclose(ts.C @ ts.C.conj().T, np.diag(dS[:ts.mCS]), atol=1e-12 * dS[0])
    assert got == {64: 46, 256: 135, 400: 155, 1024: 175}


def test_two_stage_setup_raises_past_the_kernels_atom_length(AD16):
    """s = 100 starts the rule at min(round(1.75 s log(n / s)), 400) - 1 = 399 > 256: the error names the shape."""
    Phi = _phase_code_beams(np.random.default_rng(3), 400, 256) @ AD16
    with pytest.raises(ValueError, match=r"400 x 2401 .* mCS = \d+ > 256"):
        sparse.two_stage_setup(Phi, 100)


def test_dictionary_2d_columns_and_order():
    tx, rx = 8, 4
    AD, st, sr = sparse.dictionary_2d(tx, rx)
    At, st2, _ = angular.dictionary(tx)
    Ar, sr2, _ = angular.dictionary(rx)
    assert np.array_equal(st, st2) and np.array_equal(sr, sr2) and AD.shape == (tx * rx, len(st) * len(sr))
    for u in (0, 3, len(st) - 1):
        for v in (0, 2, len(sr) - 1):
            assert np.array_equal(AD[:, u * len(sr) + v], np.kron(np.conj(At[u]), Ar[v]))
    assert np.allclose(np.linalg.norm(AD, axis=0), 1.0, atol=1e-14)
    # the synth's vec(H) order (element r + rx t): a one-path channel on the grid is one column times its gain
    u, v = 5, 7
    k = np.arange(tx * rx)
    r, t = k % rx, k // rx
    g = 0.6 - 0.8j
    h = g * np.exp(1j * angular.KAPPA * (st[u] * t - sr[v] * r))
    assert np.max(np.abs(h - g * math.sqrt(tx * rx) * AD[:, u * len(sr) + v])) <= 1e-14
    # ... and synth.channel itself is L such columns (its angles are off the grid: compare through the formula)
    aod, aoa, gains = synth.paths(5, 0, 3)
    H = synth.channel(5, 0, tx, rx, 3)
    ph = angular.KAPPA * (np.sin(np.deg2rad(aod))[None, :] * t[:, None] - np.sin(np.deg2rad(aoa))[None, :] * r[:, None])
    assert np.max(np.abs(H - (gains[None, :] * np.exp(1j * ph)).sum(axis=1))) <= 1e-13


def test_measurements_complex_has_the_modulus_measurements_returns():
    A = synth.codebook(9, 48, 64)
    for real in (0, 5):
        H = synth.channel(9, real, 8, 8, 3)
        y = synth.measurements_complex(9, real, A, H, 30.0)
        assert y.dtype == np.complex128 and np.array_equal(np.abs(y), synth.measurements(9, real, A, H, 30.0))
        w = y - A @ H
        assert 0.2 < np.mean(np.abs(w) ** 2) / 10.0 ** -3 < 5.0   # (48 draws of CN(0, 1e-3))
