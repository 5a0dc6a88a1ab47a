"""CPU tests of the beam scan's C-ABI (ace_beam_scan_batch / ace_beam_scan_host) and of its Python entry points:
the argument checks, which run before any HIP call.  No compute calls -- there is no GPU here."""
import ctypes as C

import numpy as np
import pytest

GOOD = dict(batch=1, d0=4, d1=3, Q0=5, Q1=2, K=2)


def _buffers():
    """Non-NULL dummy buffers for one realisation at the sizes of GOOD (never dereferenced: every case fails its check)."""
    return {"X": np.ones(12, np.complex128), "W0": np.ones((5, 4), np.complex128), "F1": np.ones((2, 3), np.complex128),
            "noise": None, "top_pow": np.zeros(16, np.float64), "top_idx": np.zeros(16, np.int32)}


def _call(entry, ptr, **sizes):
    from ace_amd._lib import LIB
    s = {**GOOD, **sizes}
    dims = (s["batch"], s["d0"], s["d1"], s["Q0"], s["Q1"])
    if entry == "batch":
        raw = {k: (None if v is None else v.ctypes.data) for k, v in ptr.items()}
        return LIB.ace_beam_scan_batch(*dims, raw["X"], raw["W0"], raw["F1"], raw["noise"], s["K"], raw["top_pow"],
                                       raw["top_idx"], None, None, None, None)
    dp = lambda a: None if a is None else a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ti = None if ptr["top_idx"] is None else ptr["top_idx"].ctypes.data_as(C.POINTER(C.c_int32))
    return LIB.ace_beam_scan_host(*dims, dp(ptr["X"]), dp(ptr["W0"]), dp(ptr["F1"]), dp(ptr["noise"]), s["K"],
                                  dp(ptr["top_pow"]), ti, None, None, None)


@pytest.mark.parametrize("entry", ["batch", "host"])
@pytest.mark.parametrize("name,value", [("batch", 0), ("batch", -3), ("d0", 0), ("d0", 33), ("d1", 0), ("d1", 33),
                                        ("Q0", 0), ("Q0", 4097), ("Q1", -1), ("Q1", 4097),
                                        ("K", 0), ("K", 17), ("K", 11)])   # (K = 11 > Q0 Q1 = 10)
def test_bad_sizes_are_argument_errors(entry, name, value):
    from ace_amd._lib import LIB, ACE_ERR_ARG
    assert _call(entry, _buffers(), **{name: value}) == ACE_ERR_ARG
    assert name in LIB.ace_last_error().decode()


@pytest.mark.parametrize("entry", ["batch", "host"])
@pytest.mark.parametrize("null", ["X", "W0", "F1", "top_pow", "top_idx"])
def test_null_pointers_are_argument_errors(entry, null):
    from ace_amd._lib import LIB, ACE_ERR_ARG
    ptr = _buffers()
    ptr[null] = None
    assert _call(entry, ptr) == ACE_ERR_ARG
    assert f"NULL {null}" in LIB.ace_last_error().decode()


def test_python_entry_points_exist():
    import ace_amd
    from ace_amd import angular, montecarlo, scan, synth
    for f in (ace_amd.beam_scan_host, ace_amd.beam_scan_batch, scan.beam_scan_batch, angular.steering,
              angular.dictionary, angular.quantize_ps, angular.sweep_beams, angular.estimate_angles,
              angular.beam_sweep, synth.paths, montecarlo.vs_m_baselines):
        assert callable(f)
    assert angular.ST_SWEEP == 8 and scan.K_MAX == 16
    r = ace_amd.ScanResult(np.zeros((3, 2)), np.array([[7, 0], [11, 5], [-1, -1]], np.int32), 5,
                           np.array([0, 0, 256], np.uint32))
    assert r.total is None and r.power is None and r.degenerate.tolist() == [False, False, True]
    assert r.p.tolist() == [[1, 0], [2, 1], [-1, -1]] and r.q.tolist() == [[2, 0], [1, 0], [-1, -1]]
    assert ace_amd._lib.lds_request("scan", 1) > 64 * 1024   # (past the default limit: the derived budget decides)


def test_host_entry_refuses_mismatched_shapes_and_bad_k():
    import ace_amd
    X, W0, F1 = np.ones((2, 12), complex), np.ones((5, 4), complex), np.ones((2, 3), complex)
    for bad in ((np.ones((2, 11), complex), W0, F1, 1, None),       # X is not d0 * d1 wide
                (np.ones((2, 3, 4), complex), W0, F1, 1, None),
                (X, np.ones((5, 33), complex), F1, 1, None),        # d0 > 32
                (X, W0, np.ones((2, 3, 1), complex), 1, None),
                (X, W0, F1, 0, None), (X, W0, F1, 17, None), (X, W0, F1, 11, None),
                (X, W0, F1, 1, np.ones((2, 9), complex)),           # noise is not [batch][Q1*Q0]
                (X, W0, F1, 1, np.ones((3, 10), complex))):
        with pytest.raises(ValueError):
            ace_amd.beam_scan_host(*bad)


def test_batch_entry_refuses_cpu_tensors_wrong_dtypes_and_shapes():
    import torch
    import ace_amd
    X = torch.ones((2, 12), dtype=torch.complex128)
    W0 = torch.ones((5, 4), dtype=torch.complex128)
    F1 = torch.ones((2, 3), dtype=torch.complex128)
    with pytest.raises(ValueError, match="device tensors"):
        ace_amd.beam_scan_batch(X, W0, F1)
    # the dtype and shape checks, on stand-ins that claim to be on the device (nothing is launched)
    class Dev:
        def __init__(self, t):
            self.t = t
            self.is_cuda, self.dtype, self.shape, self.device = True, t.dtype, t.shape, "cuda:0"
    with pytest.raises(TypeError):
        ace_amd.beam_scan_batch(Dev(X.to(torch.complex64)), Dev(W0), Dev(F1))
    with pytest.raises(TypeError):
        ace_amd.beam_scan_batch(Dev(X), Dev(W0), Dev(F1), noise=Dev(torch.ones((2, 10), dtype=torch.float64)))
    with pytest.raises(ValueError):
        ace_amd.beam_scan_batch(Dev(X), Dev(W0[:, :3]), Dev(F1))
    with pytest.raises(ValueError):
        ace_amd.beam_scan_batch(Dev(X), Dev(W0), Dev(F1), K=11)
    with pytest.raises(ValueError):
        ace_amd.beam_scan_batch(Dev(X), Dev(W0), Dev(F1), noise=Dev(torch.ones((2, 9), dtype=torch.complex128)))
