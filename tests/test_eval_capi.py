"""CPU tests of the channel evaluator's C-ABI (ace_evaluate_batch / ace_evaluate_host): the argument
checks, which run before any HIP call, and closed forms of the numpy restatement (tests/eval_ref.py) the
GPU tests compare against.  No compute calls -- there is no GPU here."""
import ctypes as C
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import eval_ref as ER  # noqa: E402


def _buffers():
    """Non-NULL dummy buffers for one 4 x 4 realisation (never dereferenced: every case fails its check)."""
    x = np.ones(16, np.complex128)
    g = np.ones(16, np.complex128)
    met = np.zeros(4, np.float64)
    return x, g, met


BAD_SHAPES = [(0, 4, 4), (1, 0, 4), (1, 4, 33)]


@pytest.mark.parametrize("entry", ["batch", "host"])
@pytest.mark.parametrize("batch,tx,rx", BAD_SHAPES, ids=["batch0", "tx0", "rx33"])
def test_bad_shapes_are_argument_errors(entry, batch, tx, rx):
    from ace_amd._lib import LIB, ACE_ERR_ARG
    x, g, met = _buffers()
    if entry == "batch":
        rc = LIB.ace_evaluate_batch(batch, tx, rx, x.ctypes.data, g.ctypes.data, met.ctypes.data, None, None)
    else:
        dp = lambda a: a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        rc = LIB.ace_evaluate_host(batch, tx, rx, dp(x), dp(g), dp(met), None)
    assert rc == ACE_ERR_ARG
    assert LIB.ace_last_error().decode() != ""


@pytest.mark.parametrize("entry", ["batch", "host"])
@pytest.mark.parametrize("null", ["X", "G", "metrics"])
def test_null_pointers_are_argument_errors(entry, null):
    from ace_amd._lib import LIB, ACE_ERR_ARG
    x, g, met = _buffers()
    if entry == "batch":
        ptr = {"X": x.ctypes.data, "G": g.ctypes.data, "metrics": met.ctypes.data}
        ptr[null] = None
        rc = LIB.ace_evaluate_batch(1, 4, 4, ptr["X"], ptr["G"], ptr["metrics"], None, None)
    else:
        dp = lambda a: a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        ptr = {"X": dp(x), "G": dp(g), "metrics": dp(met)}
        ptr[null] = None
        rc = LIB.ace_evaluate_host(1, 4, 4, ptr["X"], ptr["G"], ptr["metrics"], None)
    assert rc == ACE_ERR_ARG
    assert null in LIB.ace_last_error().decode()


def test_python_entry_points_exist():
    import ace_amd
    from ace_amd import montecarlo
    assert callable(ace_amd.evaluate_host) and callable(ace_amd.evaluate_batch) and callable(montecarlo.vs_m)
    r = ace_amd.EvalResult(*(np.zeros(2) for _ in range(4)), np.array([0, 256], np.uint32))
    assert r.degenerate.tolist() == [False, True]
    with pytest.raises(ValueError):
        ace_amd.evaluate_host(np.ones((2, 15)), np.ones((2, 15)), 4, 4)


# ---------------------------------------------------------------- closed forms of the helper

@pytest.mark.parametrize("tx,rx", [(1, 1), (2, 3), (8, 8), (16, 32)])
def test_scaled_truth_scores_perfectly(tx, rx):
    """x = c e^{j theta} g: nmse = 0, proj_err = 0, gain_dig = sigma1(G)."""
    rng = np.random.default_rng(100 * tx + rx)
    g = rng.standard_normal(tx * rx) + 1j * rng.standard_normal(tx * rx)
    g /= np.linalg.norm(g)
    x = 3.7 * np.exp(1.234j) * g
    nmse, _, gain_dig, proj_err = ER.evaluation_h(x, g, tx, rx)
    s1 = np.linalg.svd(ER.mat(g, tx, rx), compute_uv=False)[0]
    assert abs(nmse) <= 1e-12 and abs(proj_err) <= 1e-12 and abs(gain_dig - s1) <= 1e-12


def test_orthogonal_estimate_has_unit_nmse():
    rng = np.random.default_rng(5)
    g = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    x = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    x -= np.vdot(g, x) / np.vdot(g, g) * g
    assert abs(ER.evaluation_h(x, g, 8, 8)[0] - 1.0) <= 1e-12


@pytest.mark.parametrize("tx,rx", [(4, 4), (8, 16), (32, 32)])
def test_on_grid_rank_one_channel_reaches_the_array_gain(tx, rx):
    """G = h a b^H with the entries of a, b powers of j: the quantised beams match the channel's phases and
    gain_ana = sqrt(tx rx) |h|."""
    rng = np.random.default_rng(7 * tx + rx)
    a = 1j ** rng.integers(0, 4, tx)
    b = 1j ** rng.integers(0, 4, rx)
    h = 0.37
    G = h * np.outer(a, np.conj(b))
    g = G.T.reshape(-1)
    u1, v1 = ER.top_vectors(G)
    assert min(ER.boundary_margin(u1), ER.boundary_margin(v1)) > 0.1   # (the gauge lands on the grid)
    assert abs(ER.evaluation_h(g, g, tx, rx)[1] - np.sqrt(tx * rx) * h) <= 1e-12


def test_quantiser_ties_go_to_the_smaller_angle():
    """Quantize_PS.m:69: min returns the first entry of -pi:pi/2:pi."""
    v = np.array([1 + 1j, 1 - 1j, 1.0, -1.0 + 0j])   # angles pi/4 (tie 0 | pi/2), -pi/4 (tie -pi/2 | 0), 0, pi
    q = ER.quantize_ps(v) * 2
    np.testing.assert_allclose(q[:3], [1.0, -1j, 1.0], atol=1e-15)
    assert abs(q[3] + 1.0) <= 1e-15


def test_parity_inputs_stay_inside_the_boundary_cap():
    """The seeded parity inputs of tests/test_gpu_evaluate.py: at most 2 % of the realisations of a shape have
    an entry of u1 or v1 within 1e-6 rad of a quantisation boundary, and the metrics span the intended range."""
    for tx, rx in [(1, 1), (2, 3), (8, 8), (16, 32)]:
        X, G = ER.seeded_problem(1000 * tx + rx, 257, tx, rx)
        met, nb = ER.evaluate(X, G, tx, rx)
        assert nb.mean() <= 0.02, (tx, rx, nb.sum())
        assert np.isfinite(met).all()
        if tx * rx >= 64:
            assert met[:, 0].min() < 1e-7 and met[:, 0].max() > 1e-2
