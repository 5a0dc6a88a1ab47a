"""The scenario generator's entry points exist (C-ABI symbols and Python names), the default configuration is
ace_synth_channels' scenario, the workspace size is 0 outside the limits, and every argument and limit check answers
before any HIP call (the pointers handed in are never dereferenced).  No GPU."""
import ctypes as C
import inspect

import pytest


def test_symbols_and_names_exist():
    import ace_amd
    from ace_amd import _lib, angular, montecarlo, scenario, sparse, synth
    for sym in ("ace_scenario_cfg_default", "ace_synth_scenario_workspace_size", "ace_synth_scenario"):
        assert hasattr(_lib.LIB, sym), sym
    for name in ("scenario_batch", "ScenarioResult", "ScenarioCfg", "scenario_cfg", "scenario"):
        assert hasattr(ace_amd, name), name
    for name in ("scenario_paths", "scenario_channel", "scenario_measurements", "scenario"):
        assert callable(getattr(synth, name)), name
    assert callable(angular.kron_codebook) and callable(sparse.noisy_phase_cs) and callable(montecarlo.vs_snr)
    sig = inspect.signature(scenario.scenario_batch).parameters
    assert list(sig)[:8] == ["seed", "first", "count", "tx", "rx", "A", "cfg", "W"]
    assert sig["cfg"].default is None and sig["W"].default is None and sig["stream"].default is None
    assert set(sig["want"].default) == set(scenario.OUTPUTS) == set(f.name for f in ace_amd.ScenarioResult.__dataclass_fields__.values()) - {"noise_power"}
    sig = inspect.signature(montecarlo.vs_snr).parameters
    assert sig["methods"].default == ("A2only", "plomp", "plgamp", "perfect_cs", "noisy_cs")
    assert (sig["L"].default, sig["rician_k"].default, sig["search_deg"].default, sig["noise"].default) == (1, 5, 40.0, "combiner")
    assert sig["seed"].default is inspect.Parameter.empty and sig["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "common random numbers" in montecarlo.vs_snr.__doc__   # the stated departure from the reference's fresh draws
    assert "noise model 1" in angular.__doc__ and "keeps to the synth's" in angular.__doc__


def test_the_default_cfg_is_the_synth_channels_scenario():
    from ace_amd import synth
    from ace_amd._lib import LIB, ScenarioCfg, scenario_cfg
    cfg = ScenarioCfg()
    C.memset(C.byref(cfg), 0xFF, C.sizeof(cfg))
    LIB.ace_scenario_cfg_default(C.byref(cfg))
    assert (cfg.L, cfg.rician_k, cfg.on_grid, cfg.fix_angle, cfg.NQt, cfg.NQr, cfg.add_noise, cfg.noise_model) == (3, 0, 0, 0, 0, 0, 1, 0)
    assert (cfg.search_deg, cfg.k_factor_db, cfg.snr_db, cfg.x0_noise) == (95.0, 7.0, 30.0, 0.5)
    assert cfg.ant_d == synth.ANT_D and cfg.lambda_ == synth.LAMBDA
    assert C.sizeof(cfg) == 8 * 4 + 6 * 8
    d = synth._ScenarioDefaults
    for k, _ in ScenarioCfg._fields_:
        assert getattr(cfg, k) == getattr(d, k), k   # the mirror's defaults are the library's
    c = scenario_cfg(L=1, rician_k=5, lam=0.005)
    assert (c.L, c.rician_k, c.lambda_) == (1, 5, 0.005)
    with pytest.raises(TypeError):
        scenario_cfg(nope=1)
    LIB.ace_scenario_cfg_default(None)


def test_workspace_size_is_zero_outside_the_limits():
    from ace_amd._lib import LIB, scenario_cfg

    def size(count=4, m=32, tx=4, rx=4, Mr=0, **ck):
        cfg = scenario_cfg(**ck)
        return int(LIB.ace_synth_scenario_workspace_size(C.byref(cfg), count, m, tx, rx, Mr))

    assert size(1, 1, 1, 1) > 0 and size(4096, 4096, 32, 32) >= 4096 * (16 * 1024 + 8 * 4096)
    assert size(L=8, rician_k=16) > 0 and size(L=1, rician_k=16, NQt=65536, NQr=65536) > 0
    for bad in (dict(count=0), dict(count=-1), dict(m=0), dict(m=4097), dict(tx=0), dict(tx=33), dict(rx=0), dict(rx=33),
                dict(L=0), dict(L=9), dict(rician_k=-1), dict(rician_k=17), dict(NQt=-1), dict(NQr=65537),
                dict(noise_model=2), dict(noise_model=1, Mr=0), dict(noise_model=1, Mr=5)):
        assert size(**bad) == 0, bad
    assert LIB.ace_synth_scenario_workspace_size(None, 4, 32, 4, 4, 0) == 0
    base = size()
    assert size(count=40) > base and size(m=320) > base and size(tx=8) > base
    assert size(noise_model=1, Mr=8) > base   # the combiner noise of every realisation


def test_argument_errors_come_before_any_hip_call():
    from ace_amd._lib import LIB, scenario_cfg, ACE_ERR_ARG, ACE_ERR_UNSUPPORTED, ACE_ERR_WORKSPACE
    one = C.c_void_p(16)   # never dereferenced: the checks come first

    def call(cfg=0, first=0, count=3, m=32, tx=4, rx=4, A=one, W=None, Mr=0, ws=one, nbytes=1 << 40, **ck):
        cfg = scenario_cfg(**ck) if cfg == 0 else cfg
        return LIB.ace_synth_scenario(None if cfg is None else C.byref(cfg), 7, first, count, m, tx, rx, A, 1, W, Mr,
                                      one, one, one, one, one, one, one, one, one, ws, nbytes, None)

    err = LIB.ace_last_error
    assert call(cfg=None) == ACE_ERR_ARG and b"NULL cfg" in err()
    assert call(count=0) == ACE_ERR_ARG and b"count" in err()
    assert call(first=-1) == ACE_ERR_ARG and b"first" in err()
    assert call(tx=33) == ACE_ERR_UNSUPPORTED and b"tx 33" in err()
    assert call(rx=33) == ACE_ERR_UNSUPPORTED and b"rx 33" in err()
    assert call(m=4097) == ACE_ERR_UNSUPPORTED and b"m 4097" in err()
    assert call(L=9) == ACE_ERR_UNSUPPORTED and b"L 9" in err()
    assert call(rician_k=17) == ACE_ERR_UNSUPPORTED and b"rician_k 17" in err()
    assert call(NQt=65537) == ACE_ERR_UNSUPPORTED and call(NQr=65537) == ACE_ERR_UNSUPPORTED
    for bad in (dict(tx=0), dict(rx=0), dict(m=0), dict(L=0), dict(rician_k=-1), dict(NQt=-1), dict(NQr=-1)):
        assert call(**bad) == ACE_ERR_ARG, bad
    assert call(L=2, fix_angle=1) == ACE_ERR_ARG and b"fix_angle" in err()
    assert call(noise_model=2) == ACE_ERR_ARG and b"noise_model" in err()
    for bad in (0.0, -1.0, 181.0, float("nan")):
        assert call(search_deg=bad) == ACE_ERR_ARG and b"search_deg" in err()
    for name in ("snr_db", "k_factor_db"):
        for bad in (float("inf"), float("nan")):
            assert call(**{name: bad}) == ACE_ERR_ARG and name.encode() in err()
    for bad in (-0.5, float("inf"), float("nan")):
        assert call(x0_noise=bad) == ACE_ERR_ARG and b"x0_noise" in err()
    for name in ("ant_d", "lambda_"):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert call(**{name: bad}) == ACE_ERR_ARG and name.rstrip("_").encode() in err()
    assert call(A=None) == ACE_ERR_ARG and b"NULL A" in err()
    assert call(noise_model=1, W=None, Mr=4) == ACE_ERR_ARG and b"needs W" in err()
    assert call(noise_model=1, W=one, Mr=0) == ACE_ERR_ARG and b"Mr" in err()
    assert call(noise_model=1, W=one, Mr=5) == ACE_ERR_ARG and b"m % Mr" in err()
    assert call(ws=None) == ACE_ERR_WORKSPACE
    cfg = scenario_cfg()
    need = int(LIB.ace_synth_scenario_workspace_size(C.byref(cfg), 3, 32, 4, 4, 0))
    assert call(nbytes=need - 1) == ACE_ERR_WORKSPACE and b"workspace" in err()


def test_the_python_wrappers_check_their_inputs_without_a_device():
    import numpy as np
    from ace_amd import montecarlo, synth
    from ace_amd._lib import scenario_cfg
    with pytest.raises(ValueError, match="256"):
        montecarlo.vs_snr(8, 8, 17, [0.0], 2, seed=1)          # 289 rows: over the OMP kernel's limit, named
    with pytest.raises(ValueError):
        montecarlo.vs_snr(8, 4, 6, [0.0], 2, seed=1)           # square arrays only, as vs_m
    with pytest.raises(ValueError):
        montecarlo.vs_snr(8, 8, 6, [0.0], 2, seed=1, methods=("nope",))
    with pytest.raises(ValueError):
        montecarlo.vs_snr(8, 8, 6, [0.0], 2, seed=1, noise="pink")
    with pytest.raises(ValueError):
        synth.scenario(1, 0, 2, 9, 4, 4, np.zeros((9, 15), np.complex128))
    with pytest.raises(ValueError):
        synth.scenario_paths(1, 0, scenario_cfg(L=9))
