"""CPU tests of ace_amd.angular (grids, beams, the pure helpers) and of synth.paths, and an accuracy check of the
angular scan itself in plain numpy (tests/scan_ref.py's restatement, no GPU): on the synth's true channels the
peak of the cut dictionary's map lies within a grid step of a true path."""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import scan_ref as SR  # noqa: E402


def test_dictionary_against_the_transcribed_formula():
    """Sparse_Channel_Formulation.m:76-93 and the cut of :114-134, written out."""
    from ace_amd import angular, synth
    for n, Q, lo in ((16, 49, 8), (32, 95, 17)):
        NQ = 4 * n
        part = np.linspace(-1, 1, NQ + 1)[:-1]
        virt = 2 * np.pi * synth.ANT_D / synth.LAMBDA * part                       # :80
        edge = 2 * np.pi * synth.ANT_D / synth.LAMBDA * np.sin(np.deg2rad([-47.5, 47.5]))   # :115-117
        pos = [int(np.argmin(np.abs(virt - e))) for e in edge]                     # :119-122
        assert pos == [lo, lo + Q - 1]
        A = np.stack([np.exp(-1j * virt[u] * np.arange(n)) / np.sqrt(n) for u in range(pos[0], pos[1] + 1)])   # :86
        beams, s, deg = angular.dictionary(n)
        assert beams.shape == (Q, n) and s.shape == (Q,) and deg.shape == (Q,)
        assert np.array_equal(s, part[pos[0]:pos[1] + 1])
        np.testing.assert_allclose(beams, A, rtol=0, atol=4e-15)
        np.testing.assert_allclose(deg, np.rad2deg(np.arcsin(virt[pos[0]:pos[1] + 1] / (2 * np.pi * synth.ANT_D / synth.LAMBDA))),
                                   rtol=0, atol=1e-12)                             # Evaluation_Recovery.m:105-107
        # (the grid point nearest the edge may lie just outside it: 48.59 deg at 16 antennas)
        assert 46.5 < np.abs(deg).max() < 49.0 and np.all(np.diff(deg) > 0)
        np.testing.assert_allclose(np.abs(beams), 1 / np.sqrt(n), rtol=1e-15)
        assert angular.dictionary(n, NQ=2 * n)[0].shape[0] == {16: 25, 32: 49}[n]   # (a coarser grid, the same cut)
    assert np.array_equal(angular.steering(8, 0.0), np.full((1, 8), 1 / np.sqrt(8)))


def test_quantize_ps_values_and_ties():
    """Quantize_PS.m:63-70: the nearest of -pi : pi/2 : pi, min's first on a tie (the smaller angle)."""
    from ace_amd import angular
    ang = np.deg2rad([0, 44.9, 45.1, 90, 134, 136, 180, -44, -46, -134, -136, -179.9])
    want = [1, 1, 1j, 1j, 1j, -1, -1, 1, -1j, -1j, -1, -1]
    got = angular.quantize_ps(2.5 * np.exp(1j * ang))
    assert np.array_equal(got, np.array(want, complex))
    # exact ties: phase pi/4 between 0 and pi/2 goes to 0; -pi/4 between -pi/2 and 0 goes to -pi/2
    assert angular.quantize_ps(np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j])).tolist() == [1, -1j, 1j, -1]
    assert angular.quantize_ps(np.array([[0j]])).tolist() == [[1]]        # angle(0) = 0
    # 3 bits: unit modulus on the pi/4 grid
    q3 = angular.quantize_ps(np.exp(1j * np.deg2rad([20, 25, -100])), bits=3)
    np.testing.assert_allclose(q3, np.exp(1j * np.deg2rad([0, 45, -90])), atol=1e-15)


def test_sweep_beams_centres_and_quantisation():
    """MyBeamSweeping.m:93-108."""
    from ace_amd import angular, synth
    for n, M in ((16, 11), (16, 15), (32, 4)):
        beams, cen = angular.sweep_beams(n, M)
        part = np.linspace(-47.5, 47.5, M + 1)
        np.testing.assert_allclose(cen, (part[:-1] + part[1:]) / 2, rtol=0, atol=1e-13)
        assert beams.shape == (M, n) and set(np.unique(beams)) <= {1, -1, 1j, -1j}
        ideal = np.exp(-1j * 2 * np.pi * synth.ANT_D / synth.LAMBDA * np.sin(np.deg2rad(cen))[:, None] * np.arange(n))
        # a quantised entry is within pi / 4 of its ideal phase
        assert np.all(np.abs(np.angle(beams * ideal.conj())) <= np.pi / 4 + 1e-12)
        assert np.array_equal(beams[:, 0], np.ones(M))
    assert np.array_equal(angular.sweep_beams(16, 1)[1], [0.0])


def test_paths_reproduce_channel_bit_for_bit():
    from ace_amd import synth
    kap = 2.0 * np.pi * (synth.ANT_D / synth.LAMBDA)
    for seed, real, tx, rx, L in ((1, 0, 16, 16, 3), (7, 41, 32, 32, 1), (11, 5, 16, 16, 2), (synth.SEEDS[0], 599, 32, 32, 3)):
        aod, aoa, g = synth.paths(seed, real, L)
        assert aod.shape == aoa.shape == g.shape == (L,) and np.abs(aod).max() <= 47.5 and np.abs(aoa).max() <= 47.5
        assert abs(np.sum(np.abs(g) ** 2) - 1) < 1e-15
        sd, sa = np.sin(aod * np.pi / 180.0), np.sin(aoa * np.pi / 180.0)
        k = np.arange(tx * rx)
        r, t = k % rx, k // rx
        ph = kap * (sd[None, :] * t[:, None] - sa[None, :] * r[:, None])
        H = np.sum(g[None, :] * (np.cos(ph) + 1j * np.sin(ph)), axis=1)
        assert np.array_equal(H, synth.channel(seed, real, tx, rx, L))


def test_pure_helpers():
    from ace_amd import angular
    e = angular.aoda_err(np.array([10.0, -5.0]), np.array([0.0, 20.0]),
                         np.array([[12.0, 40.0], [30.0, -6.0]]), np.array([[1.0, 0.0], [20.0, 26.0]]))
    assert e.tolist() == [1.5, 3.5]
    g, lo, hi = angular.grid_cut(64)
    assert (lo, hi) == (8, 56) and g[0] == -1 and g[32] == 0 and g.size == 64
    # the sweep's noise depends on (seed, realisation) alone, and has the stated variance
    a = angular.sweep_noise(3, 0, 6, 4, 5, 30.0)
    b = angular.sweep_noise(3, 4, 2, 4, 5, 30.0)
    assert a.shape == (6, 20) and np.array_equal(a[4:], b) and not np.array_equal(a[0], a[1])
    assert not np.array_equal(angular.sweep_noise(4, 0, 1, 4, 5, 30.0), a[:1])
    big = angular.sweep_noise(3, 0, 4, 50, 50, 20.0)
    assert abs(np.mean(np.abs(big) ** 2) / 1e-2 - 1) < 0.05


@pytest.mark.parametrize("n,bound", [(16, 1.5), (32, 0.75)])
def test_the_cut_dictionary_finds_a_true_path(n, bound):
    """The numpy reference scan on the true channels of seed 1, realisations 0-599, L in {1, 3}: the peak's
    (|dAoD| + |dAoA|) / 2 to the nearest true path stays within ``bound`` degrees (the grid step is 1 / (2 n) in
    sin theta: at most 2.7 / 1.3 degrees between neighbours at the edge of the range, half of that to the nearest
    point, and the peak of a multi-path map moves by less than the rest).  The leaders are far apart: the GPU
    test can demand equal indices.  The full grid (no cut) is shown to alias."""
    from ace_amd import angular, synth
    Ft, _, deg_t = angular.dictionary(n)
    Wr, _, deg_r = angular.dictionary(n)
    worst, gap = 0.0, np.inf
    for L in (1, 3):
        H = np.stack([synth.channel(1, b, n, n, L) for b in range(600)])
        tr = [synth.paths(1, b, L) for b in range(600)]
        aod_t, aoa_t = np.stack([t[0] for t in tr]), np.stack([t[1] for t in tr])
        P = SR.scan(H, Wr, Ft)
        f = np.argmax(P, axis=1)
        err = angular.aoda_err(deg_t[f // Wr.shape[0]], deg_r[f % Wr.shape[0]], aod_t, aoa_t)
        top2 = -np.sort(-P, axis=1)[:, :2]
        worst, gap = max(worst, float(err.max())), min(gap, float(((top2[:, 0] - top2[:, 1]) / top2[:, 0]).min()))
        print(f"n {n} L {L}: worst {err.max():.3f} deg, median {np.median(err):.3f} deg")
    print(f"n {n}: smallest top-1 / top-2 relative gap {gap:.2e}")
    assert worst <= bound, worst
    assert gap > 1e-6, gap
    # without the cut the grid aliases: d / lambda = 0.616 > 1 / 2
    full = angular.steering(n, np.linspace(-1, 1, 4 * n + 1)[:-1])
    s = np.linspace(-1, 1, 4 * n + 1)[:-1]
    alias = np.abs(full.conj() @ full.T)
    shift = synth.LAMBDA / synth.ANT_D            # sin theta and sin theta + lambda / d give the same vector
    i = int(np.argmin(np.abs(s + 0.9)))
    j = int(np.argmin(np.abs(s - (s[i] + shift))))
    assert alias[i, j] > 0.9 and j != i
