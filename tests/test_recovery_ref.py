"""The numpy restatement of Evaluation_Recovery (tests/recovery_ref.py) against known answers.  No GPU."""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import eval_ref as ER  # noqa: E402
import recovery_ref as RR  # noqa: E402

NP = 0.1   # noise power


def _tables(tx=8, rx=4, NQ_t=32, NQ_r=16, deg=95.0):
    from ace_amd import recovery_tables
    return recovery_tables(tx, rx, NQ_t, NQ_r, deg)


def _on_grid(tb, u, v, gain=0.6 - 0.8j):
    """One path exactly on atom (u, v) of the cut grid: (the one-hot z, vecH, aod, aoa, true_idx)."""
    sc = np.sqrt(tb.tx * tb.rx)
    z = np.zeros(tb.Qt * tb.Qr, np.complex128)
    z[u * tb.Qr + v] = gain * sc
    aod, aoa = np.array([tb.deg_t[u]]), np.array([tb.deg_r[v]])
    H = gain * sc * np.outer(RR.steer(tb.rx, aoa[0], tb.kappa), np.conj(RR.steer(tb.tx, aod[0], tb.kappa)))
    return z, RR.vec(H), aod, aoa, tb.true_indices(aod[None], aoa[None])[0]


def test_the_kronecker_form_is_the_dense_product():
    from ace_amd import sparse
    tb = _tables(8, 4, 25, 16, 40.0)
    AD = sparse.dictionary_2d(8, 4, 25, 16, 40.0)[0]
    assert AD.shape == (32, tb.Qt * tb.Qr)
    rng = np.random.default_rng(0)
    z = rng.standard_normal(tb.Qt * tb.Qr) + 1j * rng.standard_normal(tb.Qt * tb.Qr)
    np.testing.assert_allclose(RR.vec(RR.channel_from_z(z, tb)), AD @ z, rtol=0, atol=1e-13)


def test_one_on_grid_path_with_the_exact_one_hot_z():
    tb = _tables()
    u, v = 5, 3
    z, h, aod, aoa, tidx = _on_grid(tb, u, v)
    assert tidx.tolist() == [[tb.first_t + u, tb.first_r + v]]
    met, he, _ = RR.evaluation_recovery(z, h, aod, aoa, tb, tidx, NP)
    assert met[0] == 0.0                       # quantisation error
    assert met[1] == 0.0 and met[2] <= 1e-28   # the estimate is the grid angle itself
    assert met[3] <= 1e-24                     # rician_k = 0: the channel is the one atom
    assert met[6] == pytest.approx(met[5], abs=1e-12)   # Rate_Est = Rate_PerCSI
    assert met[4] >= met[5] - 1e-12 and np.isnan(met[8:12]).all()
    # the truth declared 0.3 and -0.2 degrees off the atom: AoDA_Err is the grid's own offset
    met2, _, _ = RR.evaluation_recovery(z, h, aod + 0.3, aoa - 0.2, tb, tidx, NP)
    assert met2[1] == pytest.approx(0.25, abs=1e-12) and met2[0] == 0.0


def test_one_aoa_index_off_is_half_a_quantisation_step():
    tb = _tables()
    z, h, aod, aoa, tidx = _on_grid(tb, 5, 3)
    z2 = np.roll(z, 1)   # (u, v) -> (u, v + 1)
    met, _, _ = RR.evaluation_recovery(z2, h, aod, aoa, tb, tidx, NP)
    assert met[0] == 0.5
    assert met[1] == pytest.approx(0.5 * abs(tb.deg_r[4] - tb.deg_r[3]), abs=1e-12)
    tb1 = _tables(1, 4, 4, 16, 120.0)   # Nt == 1: the AoA side alone
    z, h, aod, aoa, tidx = _on_grid(tb1, 2, 3)
    met, _, _ = RR.evaluation_recovery(np.roll(z, 2), h, aod, aoa, tb1, tidx, NP)
    assert met[0] == 2.0 and met[1] == pytest.approx(abs(tb1.deg_r[5] - tb1.deg_r[3]), abs=1e-12)


def test_two_paths_and_the_no_op_of_line_128():
    """True (AoD, AoA) = (-10, 5), (20, -30).  :127 sorts the AoD to (20, -10); :128 leaves the AoA (5, -30).  The
    picks, ascending: atoms (u1, v1), (u2, v2) with u1 < u2, so the estimated AoD ascend and :131 swaps both lists."""
    tb = _tables()
    (u1, v1), (u2, v2) = (2, 6), (9, 1)
    z = np.zeros(tb.Qt * tb.Qr, np.complex128)
    z[u1 * tb.Qr + v1], z[u2 * tb.Qr + v2] = 1.0, 2.0j
    z[7] = 0.5   # a third, smaller entry that must not be picked
    aod, aoa = np.array([-10.0, 20.0]), np.array([5.0, -30.0])
    rng = np.random.default_rng(1)
    h = rng.standard_normal(32) + 1j * rng.standard_normal(32)
    met, _, _ = RR.evaluation_recovery(z, h, aod, aoa, tb, tb.true_indices(aod[None], aoa[None])[0], NP)
    eD, eA = [tb.deg_t[u2], tb.deg_t[u1]], [tb.deg_r[v2], tb.deg_r[v1]]
    err_d = (abs(eD[0] - 20.0) + abs(eD[1] + 10.0)) / 2
    err_a = (abs(eA[0] - 5.0) + abs(eA[1] + 30.0)) / 2       # against the UNSORTED true AoA
    assert met[1] == pytest.approx((err_d + err_a) / 2, abs=1e-12)
    sorted_too = (abs(eA[0] + 30.0) + abs(eA[1] - 5.0)) / 2   # what a reordering of the AoA would give
    assert abs(err_a - sorted_too) > 1.0
    assert met[0] == 0.0                                      # L > 1: no quantisation error
    # :226-227: the AoDA beams sit at the last sorted estimate, atom (u1, v1)
    G = ER.mat(h, 4, 8)
    f, w = RR.steer(8, tb.deg_t[u1], tb.kappa), RR.steer(4, tb.deg_r[v1], tb.kappa)
    g = abs(np.vdot(ER.quantize_ps(w), G @ ER.quantize_ps(f)))
    assert met[7] == pytest.approx(abs(np.log2(1 + 2 * g * g / NP)), abs=1e-12)


def test_the_determinant_identity():
    for L in (1, 2, 5):
        for g in (0.3, 2.0 - 1.0j):
            c = abs(g) ** 2 / NP
            assert np.linalg.det(np.eye(L) + c) == pytest.approx(1 + L * c, rel=1e-13)
            assert RR.rate(g, L, NP) == pytest.approx(abs(np.log2(np.linalg.det(np.eye(L) + c))), abs=1e-12)


def test_columns_13_to_15_are_evaluation_h_and_the_sweep_columns():
    from ace_amd.recovery_eval import SweepTables
    from ace_amd import angular
    tb = _tables()
    Z, H, aod, aoa, tidx = RR.seeded_problem(5, 6, tb, 2, 95.0)
    Ft, cen_t = angular.directional_beams(8, 5, 95.0)
    Wr, cen_r = angular.directional_beams(4, 3, 95.0)
    grid = angular.peak_angle_grid()
    assert len(grid) == 36001 and grid[0] == -90.0 and grid[-1] == 90.0 and grid[18000] == 0.0
    sw = SweepTables(cen_t, cen_r, RR.peak_angles(Ft, tb.kappa, grid)[0], RR.peak_angles(Wr, tb.kappa, grid)[0])
    picks = np.array([[[b % 5, b % 3], [(b + 2) % 5, (b + 1) % 3]] for b in range(6)], np.int32)
    met, He, nb = RR.evaluate(Z, H, aod, aoa, tb, tidx, NP, picks, sw)
    assert np.isfinite(met).all() and not nb.any()
    for b in range(6):
        ref = ER.evaluation_h(He[b], H[b], 4, 8)
        assert met[b, 12:].tolist() == list(ref[1:])
        assert met[b, 6] == RR.rate(ref[1], 2, NP)
        tD = np.sort(aod[b])[::-1]
        assert met[b, 11] == pytest.approx((np.mean(abs(cen_t[picks[b, 1, 0]] - tD))
                                            + np.mean(abs(cen_r[picks[b, 1, 1]] - aoa[b]))) / 2, abs=1e-12)
    # a peak angle lies within its beam's partition for these wide beams, and differs from the centre in general
    assert (np.abs(sw.peak_deg_t - cen_t) < 95.0 / 5).all()


def test_ties_go_to_the_lower_index():
    z = np.array([0.0, 3.0, 0.0, 3.0j, 0.0])
    assert RR.picks_of(z, 1).tolist() == [1] and RR.picks_of(z, 3).tolist() == [0, 1, 3]
