"""CPU tests of the held-out RSS evaluator's C-ABI (ace_rss_evaluate_batch / ace_rss_evaluate_host) and of its
Python entry points: the argument checks, which run before any HIP call.  No compute calls -- there is no GPU
here."""
import ctypes as C

import numpy as np
import pytest


def _buffers():
    """Non-NULL dummy buffers for one realisation at n = 4, Pt = 3 (never dereferenced: every case fails its check)."""
    return {"X": np.ones(4, np.complex128), "CB": np.ones((3, 4), np.complex128), "rss": np.ones(3, np.float64),
            "metrics": np.zeros(4, np.float64), "pred": np.zeros(3, np.float64)}


def _call(entry, batch, n, Pt, ptr, rss_shared=1):
    from ace_amd._lib import LIB
    if entry == "batch":
        raw = {k: (None if v is None else v.ctypes.data) for k, v in ptr.items()}
        return LIB.ace_rss_evaluate_batch(batch, n, Pt, raw["X"], raw["CB"], raw["rss"], rss_shared, raw["metrics"],
                                          raw["pred"], None, None)
    dp = lambda a: None if a is None else a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    return LIB.ace_rss_evaluate_host(batch, n, Pt, dp(ptr["X"]), dp(ptr["CB"]), dp(ptr["rss"]), rss_shared,
                                     dp(ptr["metrics"]), dp(ptr["pred"]), None)


@pytest.mark.parametrize("entry", ["batch", "host"])
@pytest.mark.parametrize("batch,n,Pt,name", [(0, 4, 3, "batch"), (-2, 4, 3, "batch"), (1, 0, 3, "n"), (1, 4, 0, "Pt"),
                                             (1, 4, -1, "Pt")])
def test_bad_sizes_are_argument_errors(entry, batch, n, Pt, name):
    from ace_amd._lib import LIB, ACE_ERR_ARG
    assert _call(entry, batch, n, Pt, _buffers()) == ACE_ERR_ARG
    assert name in LIB.ace_last_error().decode()


@pytest.mark.parametrize("entry", ["batch", "host"])
@pytest.mark.parametrize("null", ["X", "CB", "rss", "metrics"])
def test_null_pointers_are_argument_errors(entry, null):
    from ace_amd._lib import LIB, ACE_ERR_ARG
    ptr = _buffers()
    ptr[null] = None
    assert _call(entry, 1, 4, 3, ptr) == ACE_ERR_ARG
    assert f"NULL {null}" in LIB.ace_last_error().decode()


@pytest.mark.parametrize("entry", ["batch", "host"])
@pytest.mark.parametrize("shared", [-1, 2])
def test_rss_shared_must_be_zero_or_one(entry, shared):
    from ace_amd._lib import LIB, ACE_ERR_ARG
    assert _call(entry, 1, 4, 3, _buffers(), rss_shared=shared) == ACE_ERR_ARG
    assert "rss_shared" in LIB.ace_last_error().decode()


def test_python_entry_points_exist():
    import ace_amd
    from ace_amd import realtrace, rss
    from ace_amd._lib import ACE_ST_RSS_SKIPPED, ACE_ST_EVAL_DEGENERATE
    for f in (ace_amd.evaluate_rss_host, ace_amd.evaluate_rss_batch, ace_amd.dbm_to_amp, realtrace.vs_m,
              realtrace.track, realtrace.next_m, rss.evaluate_rss_batch):
        assert callable(f)
    assert ACE_ST_RSS_SKIPPED == 512 and rss.METRICS == ("mean_rel", "rms_rel", "max_rel", "n_used")
    r = ace_amd.RssEval(*(np.zeros(3) for _ in range(4)), np.array([0, 512, 256 | 512], np.uint32))
    assert r.pred is None and r.degenerate.tolist() == [False, False, True] and r.skipped.tolist() == [False, True, True]
    assert ACE_ST_EVAL_DEGENERATE == 256


def test_host_entry_refuses_mismatched_shapes():
    import ace_amd
    X, cb = np.ones((2, 6), complex), np.ones((5, 6), complex)
    for bad in ((X, np.ones((5, 7), complex), np.ones(5)),      # n differs
                (X, cb, np.ones(4)),                            # rss neither [Pt] ...
                (X, cb, np.ones((3, 5))),                       # ... nor [batch][Pt]
                (X, cb, np.ones((2, 5, 1))),
                (np.ones((2, 3, 2), complex), cb, np.ones(5))):
        with pytest.raises(ValueError):
            ace_amd.evaluate_rss_host(*bad)


def test_batch_entry_refuses_cpu_tensors_wrong_dtypes_and_shapes():
    import torch
    import ace_amd
    X = torch.ones((2, 6), dtype=torch.complex128)
    cb = torch.ones((5, 6), dtype=torch.complex128)
    rs = torch.ones(5, dtype=torch.float64)
    with pytest.raises(ValueError, match="device tensors"):
        ace_amd.evaluate_rss_batch(X, cb, rs)
    # the dtype and shape checks, on meta tensors that claim to be on the device (nothing is launched)
    class Dev:
        def __init__(self, t):
            self.t = t
            self.is_cuda, self.dtype, self.shape, self.device = True, t.dtype, t.shape, "cuda:0"
    with pytest.raises(TypeError):
        ace_amd.evaluate_rss_batch(Dev(X.to(torch.complex64)), Dev(cb), Dev(rs))
    with pytest.raises(TypeError):
        ace_amd.evaluate_rss_batch(Dev(X), Dev(cb), Dev(rs.to(torch.float32)))
    with pytest.raises(ValueError):
        ace_amd.evaluate_rss_batch(Dev(X), Dev(cb[:, :5]), Dev(rs))
    with pytest.raises(ValueError):
        ace_amd.evaluate_rss_batch(Dev(X), Dev(cb), Dev(rs[:4]))


def test_dbm_to_amp():
    import torch
    import ace_amd
    from ace_amd import engine
    dbm = np.array([-30.0, -60.0, 0.0, -47.3])
    want = np.sqrt(10.0 ** (dbm / 10.0) / 1000.0) * engine.RSS_FCT
    np.testing.assert_allclose(ace_amd.dbm_to_amp(dbm), want, rtol=1e-15)
    np.testing.assert_allclose(ace_amd.dbm_to_amp(torch.from_numpy(dbm)).numpy(), want, rtol=1e-14)
    np.testing.assert_allclose(ace_amd.dbm_to_amp(dbm, rss_fct=2.0), want * 2.0 / engine.RSS_FCT, rtol=1e-15)
    assert abs(ace_amd.dbm_to_amp(-30.0) - 1e-3 * engine.RSS_FCT) <= 1e-12   # -30 dBm = 1 uW: sqrt(1e-6) = 1e-3
