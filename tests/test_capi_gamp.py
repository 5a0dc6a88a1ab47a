"""The EM-BG-GAMP entry points exist (C-ABI symbols and Python names), the workspace size is 0 outside the limits,
and the default configuration is the PLGAMP option set of My_TwoStage_Recovery.m:165-172 with check_opts.m's
robust_gamp values.  No GPU."""
import ctypes as C
import inspect


def test_symbols_and_names_exist():
    import ace_amd
    from ace_amd import _lib, engine, gamp, montecarlo, sparse
    for sym in ("ace_gamp_cfg_default", "ace_gamp_workspace_size", "ace_gamp_solve_batch", "ace_gamp_solve_host"):
        assert hasattr(_lib.LIB, sym), sym
    for name in ("embgamp_batch", "embgamp_host", "GampResult", "ACE_ST_GAMP_NANBREAK", "ACE_ST_GAMP_MAXEM",
                 "ACE_ST_GAMP_FAILED"):
        assert hasattr(ace_amd, name), name
    assert (ace_amd.ACE_ST_GAMP_NANBREAK, ace_amd.ACE_ST_GAMP_MAXEM, ace_amd.ACE_ST_GAMP_FAILED) == (2048, 4096, 8192)
    assert callable(gamp.GampResult.channel)
    for f in (sparse.plgamp_batch, sparse.two_stage_batch, engine.recover_directional):
        assert callable(f)
    assert hasattr(engine.Engine, "channel_recovery_ADMM_v2_simulation_directional")
    assert inspect.signature(sparse.perfect_phase_cs).parameters["solver"].default == "omp"
    assert inspect.signature(montecarlo.vs_m_sparse).parameters["gamp"].default is False
    assert montecarlo.SPARSE_GAMP == ("plgamp", "perfect_cs_gamp")
    assert montecarlo.SPARSE == ("plomp", "plomp_2s", "perfect_cs")
    sig = inspect.signature(gamp.embgamp_batch).parameters
    assert sig["learn_lambda"].default is False and sig["max_em_iter"].default == 200 and sig["trace"].default is False
    # the element spacing is a parameter now, and its default is the synth's
    from ace_amd import angular
    import numpy as np
    assert np.array_equal(angular.dictionary(8)[0], angular.dictionary(8, ant_d=ace_amd.synth.ANT_D)[0])
    assert not np.array_equal(angular.steering(8, [0.3]), angular.steering(8, [0.3], ant_d=2.9e-3))
    assert sparse.dictionary_2d(4, 4, 16, 16, 180.0, 2.9e-3)[0].shape == (16, 256)


def test_workspace_size_is_zero_outside_the_limits():
    from ace_amd._lib import LIB
    assert LIB.ace_gamp_workspace_size(1, 1, 1) > 0
    assert LIB.ace_gamp_workspace_size(17, 256, 16384) >= 2 * 16 * (16384 * 144 + 256 * 112)
    for bad in ((0, 5, 7), (3, 0, 7), (3, 5, 0), (3, 257, 7), (3, 5, 16385), (-1, 5, 7)):
        assert LIB.ace_gamp_workspace_size(*bad) == 0, bad
    # realisations come in groups of 16
    assert LIB.ace_gamp_workspace_size(16, 33, 130) == LIB.ace_gamp_workspace_size(1, 33, 130)
    assert LIB.ace_gamp_workspace_size(17, 33, 130) > LIB.ace_gamp_workspace_size(16, 33, 130)


def test_the_default_cfg_is_the_plgamp_option_set():
    from ace_amd._lib import LIB, GampCfg, gamp_cfg
    cfg = GampCfg()
    C.memset(C.byref(cfg), 0xFF, C.sizeof(cfg))
    LIB.ace_gamp_cfg_default(C.byref(cfg))
    assert (cfg.learn_lambda, cfg.max_em_iter, cfg.gamp_nit, cfg.reserved) == (0, 200, 25, 0)
    assert (cfg.step0, cfg.gamp_tol, cfg.snr_db, cfg.lambda0) == (0.1, 1e-5, 0.0, 0.0)
    assert gamp_cfg(learn_lambda=1).learn_lambda == 1
