"""The host mirror of the scenario generator (ace_amd.synth.scenario_*) against properties read off
Generate_Channel.m and Generate_Measurement.m.  No GPU."""
import numpy as np
import pytest

from ace_amd import synth
from ace_amd._lib import scenario_cfg

EPS = np.finfo(np.float64).eps
KAP = 2.0 * np.pi * (synth.ANT_D / synth.LAMBDA)


def _rebuild(tx, rx, aod_deg, aoa_deg, g):
    """sum_l g_l a_rx(AoA_l) a_tx(AoD_l)^H with a(theta)[k] = exp(-1j kappa sin(theta) k) (Generate_Channel.m:117-120,
    the sqrt(Nt Nr) cancelling the two 1 / sqrt), as an rx x tx matrix."""
    H = np.zeros((rx, tx), np.complex128)
    for d, a, gl in zip(aod_deg, aoa_deg, g):
        ar = np.exp(-1j * KAP * np.sin(np.deg2rad(a)) * np.arange(rx))
        at = np.exp(-1j * KAP * np.sin(np.deg2rad(d)) * np.arange(tx))
        H += gl * np.outer(ar, at.conj())
    return H


def _mat(h, tx, rx):
    return h.reshape(tx, rx).T   # element r + rx t = H[r][t]


def test_default_cfg_is_the_synth_bit_for_bit():
    A = synth.codebook(77, 33, 35)
    for cfg in (None, scenario_cfg()):
        for real in (0, 5, 1000):
            h = synth.scenario_channel(77, real, 5, 7, cfg)
            assert np.array_equal(h, synth.channel(77, real, 5, 7))
            y, _, B, sc = synth.scenario_measurements(77, real, A, h, 7, cfg)
            assert np.array_equal(y, synth.measurements_complex(77, real, A, h))
            assert np.array_equal(B, synth.measurements(77, real, A, h))
            out = synth.scenario(77, real, 1, 33, 5, 7, A, cfg)
            x0 = synth.initial_iterate(77, real, h)
            assert np.array_equal(out["X0"][0], x0 * (1.0 / sc))   # the start itself, then the one scaling
            assert np.array_equal(out["vecH"][0], h) and out["scale"][0] == sc
    _, Bn, X0n, Hn = synth.problem(77, 5, 3, 33, 5, 7)
    out = synth.scenario(77, 5, 3, 33, 5, 7, A)
    for a, b in ((out["B"], Bn), (out["X0"], X0n), (out["Hn"], Hn)):   # x * (1 / s) against x / s
        assert np.allclose(a, b, rtol=4 * EPS, atol=0)


def test_one_path_without_nlos_is_a_rank_one_unit_modulus_matrix():
    cfg = scenario_cfg(L=1, rician_k=0, search_deg=40.0)
    for real in range(6):
        h = synth.scenario_channel(3, real, 8, 6, cfg)
        assert np.abs(np.abs(h) - 1.0).max() <= 4 * EPS
        p = synth.scenario_paths(3, real, cfg)
        assert p["flat"].shape == (4,) and abs(abs(p["gains"][0]) - 1.0) <= 2 * EPS
        assert np.abs(p["aod_deg"]).max() <= 20.0 and np.abs(p["aoa_deg"]).max() <= 20.0
        assert np.allclose(_mat(h, 8, 6), _rebuild(8, 6, p["aod_deg"], p["aoa_deg"], p["gains"]), rtol=0, atol=64 * EPS)


def test_rician_mix_rebuilds_from_paths_and_has_rank_six():
    cfg = scenario_cfg(L=1, rician_k=5, search_deg=40.0)
    K = 10.0 ** 0.7
    wd, wn = synth.k_factor_weights(cfg)
    assert wd == np.sqrt(K / (K + 1.0)) and wn == np.sqrt(1.0 / (K + 1.0)) and abs(wd * wd + wn * wn - 1.0) <= 2 * EPS
    for real in range(6):
        h = synth.scenario_channel(3, real, 8, 8, cfg)
        p = synth.scenario_paths(3, real, cfg)
        assert p["flat"].shape == (24,)
        assert abs(np.linalg.norm(p["gains"]) - 1.0) <= 4 * EPS and abs(np.linalg.norm(p["nlos_gains"]) - 1.0) <= 4 * EPS
        assert np.abs(p["nlos_aod"]).max() <= np.pi / 2 and np.abs(p["nlos_aoa"]).max() <= np.pi / 2
        H = wd * _rebuild(8, 8, p["aod_deg"], p["aoa_deg"], p["gains"]) \
            + wn * _rebuild(8, 8, np.rad2deg(p["nlos_aod"]), np.rad2deg(p["nlos_aoa"]), p["nlos_gains"])
        assert np.allclose(_mat(h, 8, 8), H, rtol=0, atol=256 * EPS)
        sv = np.linalg.svd(_mat(h, 8, 8), compute_uv=False)
        assert sv[6] < 1e-12 * sv[0] and sv[5] > 1e-9 * sv[0]
    # flat is the device's layout: AoD, AoA, gains (re, im), NLOS AoD, NLOS AoA, NLOS gains
    p = synth.scenario_paths(3, 0, cfg)
    assert np.array_equal(p["flat"][:2], [p["aod_deg"][0], p["aoa_deg"][0]])
    assert np.array_equal(p["flat"][2:4], [p["gains"][0].real, p["gains"][0].imag])
    assert np.array_equal(p["flat"][4:9], p["nlos_aod"]) and np.array_equal(p["flat"][9:14], p["nlos_aoa"])
    assert np.array_equal(p["flat"][14:], p["nlos_gains"].view(np.float64))


def test_rician_k_is_ignored_for_several_paths():
    a, b = scenario_cfg(L=3, rician_k=5), scenario_cfg(L=3, rician_k=0)
    for real in (0, 9):
        assert np.array_equal(synth.scenario_channel(11, real, 6, 4, a), synth.scenario_channel(11, real, 6, 4, b))
        assert np.array_equal(synth.scenario_channel(11, real, 6, 4, a), synth.channel(11, real, 6, 4))
        assert synth.scenario_paths(11, real, a)["flat"].shape == (12,)


@pytest.mark.parametrize("nq", [0, 20])
def test_on_grid_snaps_sin_to_the_nearest_point_first_on_a_tie(nq):
    tx, rx = 8, 5
    off, on = scenario_cfg(L=3, search_deg=120.0), scenario_cfg(L=3, search_deg=120.0, on_grid=1, NQt=nq, NQr=nq)
    for real in range(8):
        po, pg = synth.scenario_paths(5, real, off), synth.scenario_paths(5, real, on, tx, rx)
        for key, ant in (("aod_deg", tx), ("aoa_deg", rx)):
            NQ = nq or 4 * ant
            grid = np.linspace(-1.0, 1.0, NQ + 1)[:-1]
            s = np.sin(np.deg2rad(po[key]))
            want = grid[[int(np.argmin(np.abs(grid - v))) for v in s]]
            assert np.allclose(np.sin(np.deg2rad(pg[key])), want, rtol=0, atol=4 * EPS)
        assert np.array_equal(po["gains"], pg["gains"])
    # a tie goes to the first (smaller) grid point, and sin = 1 - tiny stays on the last point (the grid has no +1)
    assert synth._snap(np.array([-1.0 + 1.0 / 16, 0.999]), 16).tolist() == [-1.0, 0.875]


def test_fix_angle_gives_0_and_15_degrees_and_needs_one_path():
    cfg = scenario_cfg(L=1, fix_angle=1)
    p = synth.scenario_paths(1, 4, cfg)
    assert p["aod_deg"].tolist() == [0.0] and p["aoa_deg"].tolist() == [15.0]
    h = _mat(synth.scenario_channel(1, 4, 4, 4, cfg), 4, 4)
    assert np.allclose(h[0], h[0, 0], rtol=0, atol=8 * EPS)   # AoD = 0: constant along t
    with pytest.raises(ValueError, match="fix_angle"):
        synth.scenario_paths(1, 4, scenario_cfg(L=2, fix_angle=1))


def test_combiner_noise_repeats_per_tx_beam_and_has_the_combiners_power():
    rng = np.random.default_rng(0)
    tx, rx, Mt, Mr = 4, 4, 3, 3
    W = (rng.standard_normal((Mr, rx)) + 1j * rng.standard_normal((Mr, rx))) * 0.4
    A = synth.codebook(9, Mt * Mr, tx * rx)
    cfg = scenario_cfg(L=1, rician_k=5, noise_model=1, snr_db=10.0)
    h = synth.scenario_channel(9, 2, tx, rx, cfg)
    y = synth.scenario_measurements(9, 2, A, h, rx, cfg, W)[0]
    w = (y - A @ h).reshape(Mt, Mr)
    nz = synth.scenario_noise(9, 2, Mt * Mr, rx, cfg, W).reshape(Mt, Mr)
    assert np.array_equal(nz[0], nz[1]) and np.array_equal(nz[0], nz[2])
    assert np.allclose(w, nz, rtol=0, atol=64 * EPS)
    # noise(q) = sum_r conj(W[q][r]) N[r][q], N the stream-13 draws at counter q rx + r
    N = synth.normal_pairs(9, synth.stream_id(13, 2), Mr * rx).reshape(Mr, rx) * np.sqrt(0.1 * 0.5)
    assert np.allclose(nz[0], np.sum(W.conj() * N, axis=1), rtol=8 * EPS, atol=0)
    # mean power over 4096 realisations: sigma2 ||w_q||^2; a CN draw's power is exponential, so the standard error of
    # the mean is the mean / sqrt(4096)
    pw = np.stack([np.abs(synth.scenario_noise(9, r, Mr, rx, cfg, W)) ** 2 for r in range(4096)]).mean(axis=0)
    want = 0.1 * np.sum(np.abs(W) ** 2, axis=1)
    assert np.all(np.abs(pw - want) <= 5.0 * want / 64.0), (pw, want)
    with pytest.raises(ValueError):
        synth.scenario_noise(9, 0, 10, rx, cfg, W)      # m % Mr != 0
    assert not synth.scenario_noise(9, 0, 9, rx, scenario_cfg(add_noise=0), W).any()


def test_noisy_phase_is_the_stream_12_draw_whatever_the_snr():
    A = synth.codebook(4, 20, 24)
    h = synth.scenario_channel(4, 7, 6, 4)
    z = synth.normal_pairs(4, synth.stream_id(12, 7), 20) * np.sqrt(0.5)
    ratios = []
    for snr in (0.0, 30.0):
        y, yn, B, sc = synth.scenario_measurements(4, 7, A, h, 4, scenario_cfg(snr_db=snr))
        assert np.array_equal(yn, y * z) and np.array_equal(B, np.abs(y)) and sc == np.sqrt(np.sum(B * B))
        ratios.append(yn / y)
    assert np.allclose(ratios[0], ratios[1], rtol=8 * EPS, atol=0) and np.allclose(ratios[0], z, rtol=8 * EPS, atol=0)
    # the noise direction is shared across SNR points too (common random numbers): only sigma changes
    n0 = synth.scenario_noise(4, 7, 20, 4, scenario_cfg(snr_db=0.0))
    n30 = synth.scenario_noise(4, 7, 20, 4, scenario_cfg(snr_db=30.0))
    assert np.allclose(n0, n30 * np.sqrt(1000.0), rtol=8 * EPS, atol=0)


def test_kron_codebook_is_w_h_f_in_the_synths_order():
    from ace_amd import angular
    rng = np.random.default_rng(1)
    tx, rx, Mt, Mr = 5, 3, 4, 2
    Ft = rng.standard_normal((Mt, tx)) + 1j * rng.standard_normal((Mt, tx))
    Wr = rng.standard_normal((Mr, rx)) + 1j * rng.standard_normal((Mr, rx))
    H = rng.standard_normal((rx, tx)) + 1j * rng.standard_normal((rx, tx))
    A = angular.kron_codebook(Ft, Wr)
    assert A.shape == (Mt * Mr, tx * rx)
    got = (A @ H.T.reshape(-1)).reshape(Mt, Mr)
    want = np.array([[Wr[q].conj() @ H @ Ft[it] for q in range(Mr)] for it in range(Mt)])
    assert np.allclose(got, want, rtol=1e-13, atol=1e-13)
    assert np.array_equal(A, np.kron(Ft, Wr.conj()))
    # Directional_Beam_Angular rows scaled by 1 / sqrt(antennas) have unit norm
    B = angular.kron_codebook(angular.sweep_beams(8, 6, 40.0)[0] / np.sqrt(8), angular.sweep_beams(8, 6, 40.0)[0] / np.sqrt(8))
    assert np.allclose(np.linalg.norm(B, axis=1), 1.0, rtol=0, atol=8 * EPS)
