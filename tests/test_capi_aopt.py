"""The A-optimal selection entry points exist (C-ABI symbols and Python names), the default configuration is the
Bayes_Beam.m call's, the workspace size is 0 outside the limits, and every argument and limit check answers before any
HIP call (the pointers handed in are never dereferenced).  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest


def test_symbols_and_names_exist():
    import ace_amd
    from ace_amd import _lib, design, realtrace
    for sym in ("ace_aopt_cfg_default", "ace_aopt_workspace_size", "ace_aopt_select_batch", "ace_aopt_select_host"):
        assert hasattr(_lib.LIB, sym), sym
    for name in ("aopt_select_batch", "aopt_select_host", "bayes_beam", "AoptResult", "aopt_cfg", "ACE_ST_AOPT_SINGULAR"):
        assert hasattr(ace_amd, name), name
    assert ace_amd.ACE_ST_AOPT_SINGULAR == 65536
    # a new bit, on none of the others
    taken = [getattr(_lib, k) for k in dir(_lib) if k.startswith("ACE_ST_") and "AOPT" not in k]
    assert not any(v & 65536 for v in taken)
    sig = inspect.signature(design.aopt_select_batch).parameters
    assert (sig["kdiag"].default, sig["maxiter"].default, sig["stream"].default) == (1.0, 5, None)
    sig = inspect.signature(design.bayes_beam).parameters
    assert sig["stream_id"].default == 0 and sig["candidates"].default is None
    assert sig["seed"].default is inspect.Parameter.empty and sig["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "multiplicities" in design.bayes_beam.__doc__   # the stated departure from the reference's 40000 draws
    assert inspect.signature(realtrace.train_rows).parameters["rows"].default == "first"


def test_the_default_cfg_is_the_bayes_beam_call():
    from ace_amd._lib import LIB, AoptCfg, aopt_cfg
    cfg = AoptCfg()
    C.memset(C.byref(cfg), 0xFF, C.sizeof(cfg))
    LIB.ace_aopt_cfg_default(C.byref(cfg))
    assert (cfg.maxiter, cfg.reserved, cfg.kdiag) == (5, 0, 1.0)
    assert cfg.acutoff == -float(np.sqrt(np.finfo(np.float64).eps))
    assert aopt_cfg(maxiter=2).maxiter == 2
    with pytest.raises(TypeError):
        aopt_cfg(nope=1)
    LIB.ace_aopt_cfg_default(None)


def test_workspace_size_is_zero_outside_the_limits():
    from ace_amd._lib import LIB
    assert LIB.ace_aopt_workspace_size(1, 1, 1, 1) > 0
    assert LIB.ace_aopt_workspace_size(8, 65536, 1024, 4096) >= 8 * (16 * 1024 * 1024 + 4 * 8 * 65536)
    for bad in ((0, 64, 16, 8), (-1, 64, 16, 8), (1, 0, 16, 8), (1, 65537, 16, 8), (1, 64, 0, 8), (1, 64, 1025, 8),
                (1, 64, 16, 0), (1, 64, 16, 4097)):
        assert LIB.ace_aopt_workspace_size(*bad) == 0, bad
    # the inverses dominate and the size grows with every extent
    base = LIB.ace_aopt_workspace_size(2, 64, 16, 8)
    assert LIB.ace_aopt_workspace_size(3, 64, 16, 8) > base and LIB.ace_aopt_workspace_size(2, 6400, 16, 8) > base
    assert LIB.ace_aopt_workspace_size(2, 64, 160, 8) > base and LIB.ace_aopt_workspace_size(2, 64, 16, 800) > base


def test_argument_errors_come_before_any_hip_call():
    from ace_amd._lib import LIB, aopt_cfg, ACE_ERR_ARG, ACE_ERR_UNSUPPORTED, ACE_ERR_WORKSPACE
    one = C.c_void_p(16)   # never dereferenced: the checks come first

    def call(cfg=None, designs=3, P=64, n=16, rmax=8, F=one, nrows=one, init=one, rowlist=one, acrit=one, iters=one,
             switches=one, ws=one, nbytes=1 << 40, **ck):
        cfg = aopt_cfg(**ck) if cfg is None else cfg
        return LIB.ace_aopt_select_batch(C.byref(cfg), designs, P, n, rmax, F, nrows, init, rowlist, acrit, iters,
                                         switches, None, None, ws, nbytes, None)

    assert call(n=1025) == ACE_ERR_UNSUPPORTED and b"n 1025" in LIB.ace_last_error()
    assert call(P=65537) == ACE_ERR_UNSUPPORTED and b"P 65537" in LIB.ace_last_error()
    assert call(rmax=4097) == ACE_ERR_UNSUPPORTED and b"nrows_max 4097" in LIB.ace_last_error()
    assert call(n=0) == ACE_ERR_ARG and call(P=0) == ACE_ERR_ARG and call(rmax=0) == ACE_ERR_ARG
    assert call(designs=0) == ACE_ERR_ARG and b"designs" in LIB.ace_last_error()
    assert call(maxiter=0) == ACE_ERR_ARG and b"maxiter" in LIB.ace_last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(kdiag=bad) == ACE_ERR_ARG and b"kdiag" in LIB.ace_last_error()
    assert call(acutoff=float("nan")) == ACE_ERR_ARG and b"acutoff" in LIB.ace_last_error()
    for name in ("F", "nrows", "init", "rowlist", "acrit", "iters", "switches"):
        assert call(**{name: None}) == ACE_ERR_ARG and f"NULL {name}".encode() in LIB.ace_last_error(), name
    assert call(ws=None) == ACE_ERR_WORKSPACE
    need = int(LIB.ace_aopt_workspace_size(3, 64, 16, 8))
    assert call(nbytes=need - 1) == ACE_ERR_WORKSPACE and b"workspace" in LIB.ace_last_error()
    assert LIB.ace_aopt_select_batch(None, 3, 64, 16, 8, one, one, one, one, one, one, one, None, None, one, 1 << 40,
                                     None) == ACE_ERR_ARG and b"NULL cfg" in LIB.ace_last_error()


def test_the_host_entry_checks_nrows_and_init_before_any_hip_call():
    from ace_amd._lib import LIB, aopt_cfg, ACE_ERR_ARG
    from ace_amd import design
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert LIB.ace_aopt_select_host(None, 3, 64, 16, 8, dp(), ip(), ip(), ip(), dp(), ip(), ip(), None, None) == ACE_ERR_ARG
    F = np.zeros((64, 16), np.complex128)
    cfg = aopt_cfg()
    out = dict(rl=np.zeros((1, 8), np.int32), ac=np.zeros((1, 2)), it=np.zeros(1, np.int32), sw=np.zeros(1, np.int32))

    def host(nrows, init):
        nr, ini = np.asarray([nrows], np.int32), np.asarray([init], np.int32)
        return LIB.ace_aopt_select_host(C.byref(cfg), 1, 64, 16, 8, F.view(np.float64).ctypes.data_as(dp),
                                        nr.ctypes.data_as(ip), ini.ctypes.data_as(ip), out["rl"].ctypes.data_as(ip),
                                        out["ac"].ctypes.data_as(dp), out["it"].ctypes.data_as(ip),
                                        out["sw"].ctypes.data_as(ip), None, None)

    assert host(9, [0] * 8) == ACE_ERR_ARG and b"nrows[0] = 9" in LIB.ace_last_error()
    assert host(0, [0] * 8) == ACE_ERR_ARG
    assert host(8, [0, 1, 2, 64, 4, 5, 6, 7]) == ACE_ERR_ARG and b"init[0][3] = 64" in LIB.ace_last_error()
    assert host(3, [0, 1, -1, 64, 64, 64, 64, 64]) == ACE_ERR_ARG and b"init[0][2] = -1" in LIB.ace_last_error()
    # the Python wrappers' own shape checks
    with pytest.raises(ValueError):
        design.aopt_select_host(np.zeros((4, 1025), np.complex128), 2, [0, 1])
    with pytest.raises(ValueError):
        design.aopt_select_host(F, [2, 2], [[0, 1]])


def test_start_rows_come_from_the_counter_generator():
    from ace_amd import design, synth
    r = design.start_rows(1234, 3, 37, 64)
    assert r.dtype == np.int32 and r.shape == (64,) and r.min() >= 0 and r.max() < 37
    u = synth.u01(1234, synth.stream_id(design.ST_AOPT, 3), np.arange(64, dtype=np.uint64))
    assert np.array_equal(r, np.floor(u * 37).astype(np.int32))
    assert np.unique(r).size < 64                      # drawn with replacement
    assert not np.array_equal(r, design.start_rows(1234, 4, 37, 64))


def test_train_rows_first_and_randperm_are_unchanged():
    from ace_amd import realtrace
    from ace_amd.engine import randperm
    pool = np.array([1, 2, 4, 5, 7, 8, 9, 11, 12, 13])
    assert realtrace.train_rows(pool, 3, 0).tolist() == [1, 2, 4]
    assert realtrace.train_rows(pool, 5, 3, "randperm", seed=77).tolist() == [9, 2, 13, 12, 5]   # recorded before the change
    assert np.array_equal(realtrace.train_rows(pool, 5, 3, "randperm", seed=77), pool[randperm(77, 3, 10, 5).astype(np.int64)])
    with pytest.raises(ValueError, match="aopt"):
        realtrace.train_rows(pool, 3, 0, "aopt")       # needs the codebook
    with pytest.raises(ValueError):
        realtrace.train_rows(pool, 3, 0, "best")
