"""The min-L2 entry points exist (C-ABI symbols and Python names), the default configuration is inferMinL2.m's, the
workspace sizes are 0 outside the limits, and argument errors come back as ACE_ERR_ARG before any HIP call.  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest


def test_symbols_and_names_exist():
    import ace_amd
    from ace_amd import _lib, minl2, montecarlo
    for sym in ("ace_minl2_cfg_default", "ace_minl2_workspace_size", "ace_minl2_admm_batch", "ace_minl2_admm_host",
                "ace_minl2_solve_workspace_size", "ace_minl2_solve_batch", "ace_minl2_solve_host"):
        assert hasattr(_lib.LIB, sym), sym
    for name in ("minl2_admm_batch", "minl2_admm_host", "infer_min_l2_batch", "infer_min_l2_host", "inferMinL2",
                 "MinL2Result", "MinL2Stage", "MinL2Cfg", "minl2_cfg"):
        assert hasattr(ace_amd, name), name
    assert ace_amd.minl2 is minl2 and callable(montecarlo.vs_m_minl2)
    sig = inspect.signature(montecarlo.vs_m_minl2).parameters
    assert [k for k in sig] == ["tx", "rx", "M_list", "count", "snr_db", "L", "seed", "first", "maxiter", "device", "chunk"]
    assert sig["chunk"].default == montecarlo.CHUNK and sig["snr_db"].default == 30.0
    # vs_m and METHODS stay as they are (realtrace imports METHODS)
    assert montecarlo.METHODS == ("A2only", "A2nuclear")
    assert _lib.lds_request("minl2", 130) == 0
    # m_t = ceil(0.95 m), where the pipeline takes floor
    assert [minl2.train_count(m) for m in (16, 19, 20, 64, 1024)] == [16, 19, 19, 61, 973]


def test_the_default_cfg_is_inferMinL2s():
    from ace_amd._lib import LIB, MinL2Cfg, minl2_cfg
    cfg = MinL2Cfg()
    C.memset(C.byref(cfg), 0xFF, C.sizeof(cfg))
    LIB.ace_minl2_cfg_default(C.byref(cfg))
    assert (cfg.r, cfg.maxiter, cfg.train_seed, cfg.reserved) == (20, 500, 0, 0)
    assert (cfg.mu0, cfg.rho, cfg.cc_frac, cfg.tol_rel, cfg.tol_abs) == (1e-3, 1.03, 0.95, 1e-4, 1e-8)
    assert minl2_cfg(maxiter=40).maxiter == 40
    with pytest.raises(TypeError):
        minl2_cfg(lambda_=0.0)


def test_workspace_size_is_zero_outside_the_limits():
    from ace_amd._lib import LIB, minl2_cfg
    assert LIB.ace_minl2_workspace_size(1, 1, 1, 1) > 0
    # pinv(A) and 16 (5 m + 4 n) 32 B of state per work-group
    assert LIB.ace_minl2_workspace_size(3, 4096, 1024, 20) >= 16 * (1024 * 4096 + 3 * 32 * (5 * 4096 + 4 * 1024))
    for bad in ((0, 5, 7, 2), (3, 0, 7, 2), (3, 5, 0, 2), (3, 5, 7, 0), (3, 4097, 7, 2), (3, 5, 1025, 2), (3, 5, 7, 33),
                (-1, 5, 7, 2)):
        assert LIB.ace_minl2_workspace_size(*bad) == 0, bad
    # r > 1: one work-group per realisation; r = 1: one per 32 realisations
    assert LIB.ace_minl2_workspace_size(2, 48, 16, 16) > LIB.ace_minl2_workspace_size(1, 48, 16, 16)
    assert LIB.ace_minl2_workspace_size(32, 48, 16, 1) == LIB.ace_minl2_workspace_size(1, 48, 16, 1)
    assert LIB.ace_minl2_workspace_size(33, 48, 16, 1) > LIB.ace_minl2_workspace_size(32, 48, 16, 1)
    cfg = minl2_cfg()
    assert LIB.ace_minl2_solve_workspace_size(C.byref(cfg), 4, 64, 16) > 0
    for bad in ((0, 64, 16), (4, 0, 16), (4, 64, 0), (4, 4097, 16), (4, 64, 1025)):
        assert LIB.ace_minl2_solve_workspace_size(C.byref(cfg), *bad) == 0, bad
    assert LIB.ace_minl2_solve_workspace_size(None, 4, 64, 16) == 0
    assert LIB.ace_minl2_solve_workspace_size(C.byref(minl2_cfg(r=0)), 4, 64, 16) == 0


def _stage(cfg, batch, m, n, r, sbr, A, B, X0, X, Y, ws=None, nws=0):
    from ace_amd._lib import LIB
    return LIB.ace_minl2_admm_batch(cfg, batch, m, n, r, sbr, A, B, X0, None, X, Y, None, None, None, None, None, None,
                                    ws, nws, None)


def test_argument_errors_come_before_any_hip_call():
    from ace_amd._lib import LIB, ACE_ERR_ARG, ACE_ERR_WORKSPACE, minl2_cfg
    cfg = C.byref(minl2_cfg())
    p = 0x1000   # never dereferenced: every call below fails on its arguments
    assert _stage(None, 1, 8, 4, 2, 1, p, p, p, p, p) == ACE_ERR_ARG and b"cfg" in LIB.ace_last_error()
    for k, name in enumerate(("A", "B", "X0", "X", "Y")):
        ptrs = [p] * 5
        ptrs[k] = None
        assert _stage(cfg, 1, 8, 4, 2, 1, *ptrs) == ACE_ERR_ARG
        assert LIB.ace_last_error().decode().endswith("NULL " + name)
    for batch, m, n, r in ((0, 8, 4, 2), (1, 0, 4, 2), (1, 8, 0, 2), (1, 8, 4, 0), (1, 4097, 4, 2), (1, 8, 1025, 2),
                           (1, 8, 4, 33)):
        assert _stage(cfg, batch, m, n, r, 1, p, p, p, p, p) == ACE_ERR_ARG, (batch, m, n, r)
    assert _stage(cfg, 1, 8, 4, 2, 2, p, p, p, p, p) == ACE_ERR_ARG
    for kw in (dict(maxiter=0), dict(mu0=0.0), dict(rho=-1.0), dict(tol_rel=-1e-4), dict(tol_abs=float("nan"))):
        assert _stage(C.byref(minl2_cfg(**kw)), 1, 8, 4, 2, 1, p, p, p, p, p) == ACE_ERR_ARG, kw
    assert _stage(cfg, 1, 8, 4, 2, 1, p, p, p, p, p, None, 0) == ACE_ERR_WORKSPACE
    assert _stage(cfg, 1, 8, 4, 2, 1, p, p, p, p, p, p, 16) == ACE_ERR_WORKSPACE
    # the whole recovery
    solve = lambda c, batch, m, n, A, B, tr, X, Y: LIB.ace_minl2_solve_batch(  # noqa: E731
        c, batch, m, n, A, B, tr, X, Y, None, None, None, None, None, 0, None)
    assert solve(None, 1, 8, 4, p, p, None, p, p) == ACE_ERR_ARG
    for k in range(4):
        ptrs = [p] * 4
        ptrs[k] = None
        assert solve(cfg, 1, 8, 4, ptrs[0], ptrs[1], None, ptrs[2], ptrs[3]) == ACE_ERR_ARG
    for batch, m, n in ((0, 8, 4), (1, 0, 4), (1, 8, 0), (1, 4097, 4), (1, 8, 1025)):
        assert solve(cfg, batch, m, n, p, p, None, p, p) == ACE_ERR_ARG
    assert solve(C.byref(minl2_cfg(cc_frac=0.0)), 1, 8, 4, p, p, None, p, p) == ACE_ERR_ARG
    assert solve(C.byref(minl2_cfg(r=0)), 1, 8, 4, p, p, None, p, p) == ACE_ERR_ARG
    ip = lambda a: np.asarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    for tr in ([0, 1, 2, 3, 4, 5, 6, 6], [0, 1, 2, 3, 4, 5, 6, 8], [-1, 1, 2, 3, 4, 5, 6, 7]):   # m_t = ceil(7.6) = 8
        assert solve(cfg, 1, 8, 4, p, p, ip(tr), p, p) == ACE_ERR_ARG and b"train_idx" in LIB.ace_last_error()
    assert solve(cfg, 1, 8, 4, p, p, ip(range(8)), p, p) == ACE_ERR_WORKSPACE


def test_the_python_wrappers_check_shapes():
    from ace_amd import minl2
    A, B = np.ones((8, 4), complex), np.ones((2, 8))
    with pytest.raises(ValueError):
        minl2.minl2_admm_host(A, B, np.ones((2, 3, 5), complex), scale_by_row=True)
    with pytest.raises(ValueError):
        minl2.minl2_admm_host(A, B, np.ones((2, 33, 4), complex), scale_by_row=True)
    with pytest.raises(ValueError):
        minl2.minl2_admm_host(A, B, np.ones((2, 3, 4), complex), scale_by_row=True, rcols=[1])
    with pytest.raises(ValueError):
        minl2.infer_min_l2_host(A, B, np.arange(7))
    with pytest.raises(ValueError):
        minl2.inferMinL2(A, B[0], 0.5)
