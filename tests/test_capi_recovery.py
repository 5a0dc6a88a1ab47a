"""The recovery evaluator's entry points exist (C-ABI symbols and Python names), the column order is the reference's,
the per-call tables are the cut dictionaries', and every argument and limit check answers before any HIP call (the
pointers handed in are never dereferenced).  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest


def test_symbols_and_names_exist():
    import ace_amd
    from ace_amd import _lib, angular, montecarlo, recovery_eval
    for sym in ("ace_evaluate_recovery_batch", "ace_evaluate_recovery_host", "ace_beam_peak_angles",
                "ace_beam_peak_angles_host"):
        assert hasattr(_lib.LIB, sym), sym
    for name in ("evaluate_recovery_host", "evaluate_recovery_batch", "recovery_tables", "sweep_tables",
                 "METRICS_RECOVERY", "RecoveryEval", "ACE_ST_RECEVAL_NOSWEEP"):
        assert hasattr(ace_amd, name), name
    assert ace_amd.METRICS_RECOVERY == (
        "num_quantization_error", "aoda_err", "mse_arm", "mse_h", "rate_unconstrained", "rate_percsi", "rate_est",
        "rate_est_aoda", "rate_bsweep1", "rate_bsweep2", "aoda_err_sweep1", "aoda_err_sweep2", "gain_ana", "gain_dig",
        "proj_error")
    assert recovery_eval.NCOL == 15 and _lib.ACE_ST_RECEVAL_NOSWEEP == 131072
    assert callable(angular.directional_beams) and callable(angular.beam_peak_angles)
    assert callable(montecarlo.vs_sr)
    sig = inspect.signature(montecarlo.vs_sr).parameters
    assert list(sig)[:6] == ["tx", "rx", "area_list", "M_lists", "G_lists", "count"]
    assert sig["methods"].default == ("plomp", "plgamp", "perfect_cs", "noisy_cs")
    assert (sig["snr_db"].default, sig["rician_k"].default) == (0.0, 5)
    assert sig["seed"].default is inspect.Parameter.empty and sig["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    for f in (montecarlo.vs_m_sparse, montecarlo.vs_snr):
        assert inspect.signature(f).parameters["columns"].default == "h"
    r = ace_amd.RecoveryEval(np.arange(30.0).reshape(2, 15), np.array([0, 256 | 131072], np.uint32))
    assert r.mse_h.tolist() == [3.0, 18.0] and r.proj_error.tolist() == [14.0, 29.0]
    assert r.degenerate.tolist() == [False, True] and r.no_sweep.tolist() == [False, True]
    with pytest.raises(AttributeError):
        r.nope


def test_directional_beams_are_the_sweep_beams():
    from ace_amd import angular
    for n, M, deg in ((12, 7, 40.0), (4, 3, 20.0)):
        a, b = angular.directional_beams(n, M, deg), angular.sweep_beams(n, M, deg)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.allclose(np.abs(a[0]), 1.0)
    assert "alias" in angular.directional_beams.__doc__
    g = angular.peak_angle_grid()
    assert g.shape == (36001,) and g[0] == -90.0 and g[-1] == 90.0 and (np.diff(g) > 0).all()


def test_the_tables_are_the_cut_dictionaries():
    from ace_amd import angular, recovery_tables, sparse
    tb = recovery_tables(8, 4, 25, 16, 40.0)
    At, st, dt = angular.dictionary(8, 25, 40.0)
    Ar, sr, dr = angular.dictionary(4, 16, 40.0)
    assert np.array_equal(tb.A_t, At) and np.array_equal(tb.A_r, Ar)
    assert np.array_equal(tb.deg_t, dt) and np.array_equal(tb.deg_r, dr)
    assert tb.Qt * tb.Qr == sparse.dictionary_2d(8, 4, 25, 16, 40.0)[0].shape[1]
    assert np.array_equal(tb.grid_t[tb.first_t:tb.first_t + tb.Qt], st)
    assert np.array_equal(tb.grid_r[tb.first_r:tb.first_r + tb.Qr], sr)
    assert tb.kappa == angular.KAPPA
    # the nearest global index: on the grid it is the point itself, and a tie goes to the first
    idx = tb.true_indices(dt[None, :3], dr[None, :3])
    assert idx.shape == (1, 3, 2) and idx.dtype == np.int32
    assert idx[0, :, 0].tolist() == [tb.first_t + k for k in range(3)]
    assert idx[0, :, 1].tolist() == [tb.first_r + k for k in range(3)]
    mid = np.rad2deg(np.arcsin(0.5 * (tb.grid_r[8] + tb.grid_r[9])))   # 0.0625: exactly between two points
    assert tb.true_indices(np.array([[0.0]]), np.array([[mid]]))[0, 0, 1] in (8, 9)
    # with a scenario's paths the true angles and indices are attached
    paths = np.array([[10.0, -5.0, 3.0, 7.0, 1, 0, 0, 1]])
    t2 = recovery_tables(8, 4, 25, 16, 40.0, paths=paths, L=2)
    assert t2.aod_deg.tolist() == [[10.0, -5.0]] and t2.aoa_deg.tolist() == [[3.0, 7.0]]
    assert np.array_equal(t2.true_idx, tb.true_indices(t2.aod_deg, t2.aoa_deg))
    with pytest.raises(ValueError):
        recovery_tables(8, 4, paths=paths)


def test_argument_errors_come_before_any_hip_call():
    from ace_amd._lib import LIB, ACE_ERR_ARG, ACE_ERR_UNSUPPORTED
    one = C.c_void_p(16)   # never dereferenced: the checks come first

    def call(batch=3, tx=4, rx=4, L=1, Qt=8, Qr=8, first_t=0, first_r=0, noise=0.1, kappa=3.87, picks=None, Mt=0,
             Mr=0, tables=None, **null):
        p = {k: one for k in ("A_t", "A_r", "deg_t", "deg_r", "z", "vecH", "aod", "aoa", "tidx", "metrics")}
        p.update({k: None for k in null})
        t = [tables] * 4
        return LIB.ace_evaluate_recovery_batch(batch, tx, rx, L, Qt, Qr, p["A_t"], p["A_r"], p["deg_t"], p["deg_r"],
                                               first_t, first_r, noise, kappa, p["z"], p["vecH"], p["aod"], p["aoa"],
                                               p["tidx"], picks, Mt, Mr, *t, p["metrics"], None, None, None)

    err = LIB.ace_last_error
    assert call(batch=0) == ACE_ERR_ARG and b"batch" in err()
    assert call(tx=0) == ACE_ERR_ARG and call(rx=0) == ACE_ERR_ARG
    assert call(tx=33) == ACE_ERR_UNSUPPORTED and b"tx 33" in err()
    assert call(rx=33) == ACE_ERR_UNSUPPORTED and b"rx 33" in err()
    assert call(L=0) == ACE_ERR_ARG and b"L 0" in err()
    assert call(L=9) == ACE_ERR_UNSUPPORTED and b"L 9" in err()
    assert call(Qt=0) == ACE_ERR_ARG and call(Qr=0) == ACE_ERR_ARG
    assert call(Qt=4097) == ACE_ERR_UNSUPPORTED and b"Qt 4097" in err()
    assert call(Qr=4097) == ACE_ERR_UNSUPPORTED and b"Qr 4097" in err()
    assert call(L=5, Qt=2, Qr=2) == ACE_ERR_ARG and b"atoms" in err()
    assert call(first_t=-1) == ACE_ERR_ARG and call(first_r=-1) == ACE_ERR_ARG and b"first" in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(noise=bad) == ACE_ERR_ARG and b"noise_power" in err()
        assert call(kappa=bad) == ACE_ERR_ARG and b"kappa" in err()
    for k, name in (("A_t", b"A_t"), ("A_r", b"A_r"), ("deg_t", b"deg_t"), ("deg_r", b"deg_r"), ("z", b"NULL z"),
                    ("vecH", b"vecH"), ("aod", b"aod_deg"), ("aoa", b"aoa_deg"), ("tidx", b"true_idx"),
                    ("metrics", b"metrics")):
        assert call(**{k: None}) == ACE_ERR_ARG and name in err(), k
    assert call(picks=one, Mt=0, Mr=3, tables=one) == ACE_ERR_ARG and b"Mt 0" in err()
    assert call(picks=one, Mt=3, Mr=4097, tables=one) == ACE_ERR_UNSUPPORTED
    assert call(picks=one, Mt=3, Mr=3, tables=None) == ACE_ERR_ARG and b"tables" in err()
    # the host entry runs the same checks first
    d = C.POINTER(C.c_double)()
    i = C.POINTER(C.c_int32)()
    assert LIB.ace_evaluate_recovery_host(0, 4, 4, 1, 8, 8, d, d, d, d, 0, 0, 0.1, 3.87, d, d, d, d, i, i, 0, 0, d, d,
                                          d, d, d, d, None) == ACE_ERR_ARG
    # the peak angles
    assert LIB.ace_beam_peak_angles(0, 4, 3.87, one, one, None) == ACE_ERR_ARG and b"M 0" in err()
    assert LIB.ace_beam_peak_angles(2, 0, 3.87, one, one, None) == ACE_ERR_ARG
    assert LIB.ace_beam_peak_angles(2, 33, 3.87, one, one, None) == ACE_ERR_UNSUPPORTED and b"N 33" in err()
    assert LIB.ace_beam_peak_angles(2, 4, 0.0, one, one, None) == ACE_ERR_ARG and b"kappa" in err()
    assert LIB.ace_beam_peak_angles(2, 4, 3.87, None, one, None) == ACE_ERR_ARG and b"beams" in err()
    assert LIB.ace_beam_peak_angles(2, 4, 3.87, one, None, None) == ACE_ERR_ARG and b"peak_deg" in err()


def test_the_python_wrappers_check_their_inputs_without_a_device():
    from ace_amd import evaluate_recovery_host, montecarlo, recovery_tables
    tb = recovery_tables(4, 4, 16, 16, 120.0)
    n = tb.Qt * tb.Qr
    z, h, a = np.zeros((2, n), complex), np.zeros((2, 16), complex), np.zeros((2, 1))
    with pytest.raises(ValueError, match="Qt"):
        evaluate_recovery_host(z[:, :-1], h, a, a, tb, noise_power=0.1)
    with pytest.raises(ValueError, match="vecH"):
        evaluate_recovery_host(z, h[:, :-1], a, a, tb, noise_power=0.1)
    with pytest.raises(ValueError, match="aod_deg"):
        evaluate_recovery_host(z, h, np.zeros((2, 9)), np.zeros((2, 9)), tb, noise_power=0.1)
    with pytest.raises(ValueError, match="go together"):
        evaluate_recovery_host(z, h, a, a, tb, noise_power=0.1, picks=np.zeros((2, 2, 2), np.int32))
    with pytest.raises(ValueError, match="noise_power"):
        evaluate_recovery_host(z, h, a, a, tb, noise_power=0.0)
    with pytest.raises(TypeError):
        evaluate_recovery_host(z, h, a, a, None, noise_power=0.1)
    with pytest.raises(ValueError):
        montecarlo.vs_sr(4, 4, (20,), ((2, 3),), ((16,),), 2, seed=1)            # M and G lists must pair up
    with pytest.raises(ValueError):
        montecarlo.vs_sr(4, 4, (20,), ((2,),), ((16,),), 2, seed=1, methods=("nope",))
    with pytest.raises(ValueError):
        montecarlo.vs_sr(8, 4, (20,), ((2,),), ((16,),), 2, seed=1)              # square arrays only, as vs_snr
    with pytest.raises(ValueError):
        montecarlo.vs_m_sparse(4, 4, [16], 2, seed=1, columns="nope")
    with pytest.raises(ValueError):
        montecarlo.vs_snr(4, 4, 3, [0.0], 2, seed=1, columns="nope")
