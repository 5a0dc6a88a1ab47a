"""The PR-GAMP entry points exist (C-ABI symbols and Python names), the default configuration is the option set of
MyCPR.m:110-120, the workspace size is 0 outside the limits, and every argument and limit check answers before any HIP
call (the pointers handed in are never dereferenced).  The host twin of the generated restart draws follows the
counter layout ace_amd/prgamp.py states.  No GPU."""
import ctypes as C
import inspect

import numpy as np


def test_symbols_and_names_exist():
    import ace_amd
    from ace_amd import _lib, montecarlo, prgamp
    for sym in ("ace_prgamp_cfg_default", "ace_prgamp_workspace_size", "ace_prgamp_solve_batch", "ace_prgamp_solve_host"):
        assert hasattr(_lib.LIB, sym), sym
    for name in ("prgamp_batch", "prgamp_host", "PrGampResult", "prgamp_cfg", "ACE_ST_PRGAMP_FAILED", "ACE_ST_PRGAMP_MAXTRY"):
        assert hasattr(ace_amd, name), name
    assert (ace_amd.ACE_ST_PRGAMP_FAILED, ace_amd.ACE_ST_PRGAMP_MAXTRY) == (16384, 32768)
    # new bits, next to the GAMP ones and on none of theirs
    taken = [getattr(_lib, k) for k in dir(_lib) if k.startswith("ACE_ST_") and "PRGAMP" not in k]
    assert not any(v & (16384 | 32768) for v in taken)
    sig = inspect.signature(prgamp.prgamp_batch).parameters
    assert (sig["max_try"].default, sig["nit_em"].default, sig["gamp_nit"].default) == (100, 50, 200)
    assert sig["draws"].default is None and sig["seed"].default is None
    assert inspect.signature(montecarlo.vs_m_sparse).parameters["prgamp"].default is False
    assert montecarlo.SPARSE_PRGAMP == ("prgamp",)
    assert _lib.lds_request("prgamp", 256) == 98688 and _lib.lds_request("prgamp", 1) == 98304


def test_the_default_cfg_is_the_mycpr_option_set():
    from ace_amd._lib import LIB, PrGampCfg, prgamp_cfg
    cfg = PrGampCfg()
    C.memset(C.byref(cfg), 0xFF, C.sizeof(cfg))
    LIB.ace_prgamp_cfg_default(C.byref(cfg))
    assert (cfg.max_try, cfg.nit_em, cfg.gamp_nit, cfg.reserved) == (100, 50, 200, 0)
    assert (cfg.sparse_rat, cfg.snr_db_init, cfg.snr_db) == (0.0, 20.0, 25.0)
    assert prgamp_cfg(max_try=3).max_try == 3
    LIB.ace_prgamp_cfg_default(None)


def test_workspace_size_is_zero_outside_the_limits():
    from ace_amd._lib import LIB
    assert LIB.ace_prgamp_workspace_size(1, 1, 1, 1) > 0
    assert LIB.ace_prgamp_workspace_size(17, 256, 16384, 100) >= 2 * 16 * (16384 * 184 + 256 * 192)
    for bad in ((0, 5, 7, 1), (3, 0, 7, 1), (3, 5, 0, 1), (3, 257, 7, 1), (3, 5, 16385, 1), (-1, 5, 7, 1), (3, 5, 7, 0)):
        assert LIB.ace_prgamp_workspace_size(*bad) == 0, bad
    # realisations come in groups of 16; the draws are the caller's, so max_try does not enter
    assert LIB.ace_prgamp_workspace_size(16, 33, 130, 2) == LIB.ace_prgamp_workspace_size(1, 33, 130, 2)
    assert LIB.ace_prgamp_workspace_size(17, 33, 130, 2) > LIB.ace_prgamp_workspace_size(16, 33, 130, 2)
    assert LIB.ace_prgamp_workspace_size(17, 33, 130, 2) == LIB.ace_prgamp_workspace_size(17, 33, 130, 100)


def test_argument_errors_come_before_any_hip_call():
    from ace_amd._lib import LIB, prgamp_cfg, ACE_ERR_ARG, ACE_ERR_UNSUPPORTED, ACE_ERR_WORKSPACE
    one = C.c_void_p(16)   # never dereferenced: the checks come first
    good = dict(sparse_rat=0.1)

    def call(cfg=None, batch=3, m=5, N=7, G=one, xhat=one, info=one, ws=one, nbytes=1 << 30, **ck):
        cfg = prgamp_cfg(**{**good, **ck}) if cfg is None else cfg
        return LIB.ace_prgamp_solve_batch(C.byref(cfg), batch, m, N, one, one, G, xhat, info, one, None, None, None, ws,
                                          nbytes, None)

    assert call(m=257) == ACE_ERR_UNSUPPORTED and b"m 257" in LIB.ace_last_error()
    assert call(N=16385) == ACE_ERR_UNSUPPORTED
    assert call(m=0) == ACE_ERR_ARG and call(N=0) == ACE_ERR_ARG and call(batch=0) == ACE_ERR_ARG
    assert call(sparse_rat=0.0) == ACE_ERR_ARG and b"sparse_rat" in LIB.ace_last_error()
    assert call(sparse_rat=1.5) == ACE_ERR_ARG and call(sparse_rat=float("nan")) == ACE_ERR_ARG
    assert call(snr_db=float("inf")) == ACE_ERR_ARG and call(snr_db_init=float("nan")) == ACE_ERR_ARG
    assert call(max_try=0) == ACE_ERR_ARG and b"max_try" in LIB.ace_last_error()
    assert call(nit_em=-1) == ACE_ERR_ARG and b"nit_em" in LIB.ace_last_error()
    assert call(gamp_nit=0) == ACE_ERR_ARG and b"gamp_nit" in LIB.ace_last_error()
    assert call(xhat=None) == ACE_ERR_ARG and b"NULL xhat" in LIB.ace_last_error()
    assert call(G=None) == ACE_ERR_ARG and b"NULL G" in LIB.ace_last_error()
    assert call(info=None) == ACE_ERR_ARG
    assert call(ws=None) == ACE_ERR_WORKSPACE
    need = int(LIB.ace_prgamp_workspace_size(3, 5, 7, 100))
    assert call(nbytes=need - 1) == ACE_ERR_WORKSPACE and b"workspace" in LIB.ace_last_error()
    assert LIB.ace_prgamp_solve_batch(None, 3, 5, 7, one, one, one, one, one, one, None, None, None, one, 1 << 30,
                                      None) == ACE_ERR_ARG
    dp = C.POINTER(C.c_double)
    assert LIB.ace_prgamp_solve_host(None, 3, 5, 7, dp(), dp(), dp(), dp(), dp(), None, None, None, None) == ACE_ERR_ARG


def test_the_generated_draws_follow_the_stated_counter_layout():
    """Realisation b, try t, atom j: the Box-Muller pair of counters 2 c, 2 c + 1 (c = t N + j) of stream
    stream_id(ST_PRGAMP, first + b).  The torch generator (here on the CPU device) and the host twin use the same
    integers; the floating-point step agrees to rounding."""
    import torch
    from ace_amd import prgamp, synth
    seed, batch, T, N = 1234567, 3, 2, 5
    h = prgamp.prgamp_draws_host(seed, batch, T, N, first=4)
    assert h.shape == (batch, T, N) and h.dtype == np.complex128
    b, t, j = 2, 1, 3
    c = np.uint64(t * N + j)
    st = synth.stream_id(prgamp.ST_PRGAMP, 4 + b)
    u1, u2 = synth.u01(seed, st, 2 * c), synth.u01(seed, st, 2 * c + np.uint64(1))
    r = np.sqrt(-2.0 * np.log(1.0 - u1))
    assert h[b, t, j] == complex(r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2))
    g = prgamp.prgamp_draws(seed, batch, T, N, torch.device("cpu"), first=4).numpy()
    assert np.allclose(g, h, rtol=1e-13, atol=1e-15)
    big = prgamp.prgamp_draws_host(99, 1, 4, 4096)
    assert abs(big.real.var() - 1.0) < 0.05 and abs(big.imag.var() - 1.0) < 0.05 and abs(big.mean()) < 0.05
