"""ace_synth_scenario on the GPU against the host mirror (ace_amd.synth.scenario) and against its own defining
formulas, at shapes whose tails leave the 16 x 16 tiles partly empty."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SEED, FIRST = 4242, 5
OUTS = ("vecH", "y", "y_noisy", "B_raw", "scale", "B", "X0", "Hn", "paths")

# name: (count, m, tx, rx, shared, cfg fields, Mr)
CASES = {
    "rician_17x33": (17, 33, 5, 7, True, dict(L=1, rician_k=5, search_deg=40.0, snr_db=10.0), 0),
    "combiner_3x9": (3, 9, 4, 4, True, dict(L=1, rician_k=5, search_deg=40.0, snr_db=5.0, noise_model=1), 3),
    "private_5x20": (5, 20, 6, 4, False, dict(L=3, on_grid=1, search_deg=120.0, snr_db=20.0), 0),
    "big_3x256": (3, 256, 32, 32, True, dict(L=1, rician_k=16, search_deg=120.0, snr_db=30.0), 0),
    "default_17x33": (17, 33, 5, 7, True, {}, 0),
    "default_3x256": (3, 256, 32, 32, True, {}, 0),
}
MAIN = ("rician_17x33", "combiner_3x9", "private_5x20", "big_3x256")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(A [1 or count][m][n], W or None) on the host: the phase-code codebook(s) of the synth, or for the combiner case
    the Kronecker codebook of 3 x 3 directional beams."""
    from ace_amd import angular, synth
    count, m, tx, rx, shared, _, Mr = CASES[name]
    if Mr:
        Ft, Wr = angular.sweep_beams(tx, m // Mr, 40.0)[0] / np.sqrt(tx), angular.sweep_beams(rx, Mr, 40.0)[0] / np.sqrt(rx)
        return angular.kron_codebook(Ft, Wr)[None], Wr
    if shared:
        return synth.codebook(SEED, m, tx * rx)[None], None
    return np.stack([synth.codebook(SEED, m, tx * rx, FIRST + c) for c in range(count)]), None


def _cfg(name):
    from ace_amd._lib import scenario_cfg
    return scenario_cfg(**CASES[name][5])


def _run(name, first=FIRST, count=None, rows=None, want=OUTS, stream=None, workspace=None):
    """One scenario_batch call; ``rows``: the codebooks of a private case to pass (a slice)."""
    import torch
    from ace_amd import scenario_batch
    n_all, m, tx, rx, shared, _, _ = CASES[name]
    A, W = _inputs(name)
    dev = torch.device("cuda:0")
    Ad = torch.from_numpy(A if shared or rows is None else np.ascontiguousarray(A[rows])).to(dev)
    Wd = None if W is None else torch.from_numpy(W).to(dev)
    res = scenario_batch(SEED, first, n_all if count is None else count, tx, rx, Ad, _cfg(name), Wd, want=want,
                         stream=stream, workspace=workspace, a_shared=shared)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    return {k: getattr(res, k).cpu().numpy() for k in want}


@functools.lru_cache(maxsize=None)
def _device(name):
    return _run(name)


@functools.lru_cache(maxsize=None)
def _mirror(name):
    from ace_amd import synth
    count, m, tx, rx, _, _, _ = CASES[name]
    A, W = _inputs(name)
    return synth.scenario(SEED, FIRST, count, m, tx, rx, A, _cfg(name), W)


@pytest.mark.parametrize("name", MAIN)
def test_channel_and_start_match_the_mirror(gpu, name):
    d, h = _device(name), _mirror(name)
    for k in ("vecH", "X0", "Hn"):   # test_device_synth_matches_host's tolerances for the same quantities
        assert np.allclose(d[k], h[k], rtol=1e-11, atol=1e-13), k
    assert np.isfinite(d["scale"]).all() and (d["scale"] > 0).all()


@pytest.mark.parametrize("name", MAIN)
def test_paths_match_the_mirror_to_rounding(gpu, name):
    """The draws are the same counter values on both sides; what differs is the rounding of log, sqrt, sincos, sin,
    asin and the divisions in two math libraries, each within 2 ulp: at most 8 operations lie between a counter value
    and a stored number, so 16 eps.  An angle is bounded relative to itself, a gain relative to its modulus (its parts
    are r cos and r sin of a phase that is the same on both sides)."""
    from ace_amd.scenario import rician_in_effect
    d, h = _device(name)["paths"], _mirror(name)["paths"]
    cfg = _cfg(name)
    L, Rk = cfg.L, rician_in_effect(cfg)
    assert d.shape == h.shape == (CASES[name][0], 4 * (L + Rk))
    ang = np.r_[0:2 * L, 4 * L:4 * L + 2 * Rk]
    worst = np.max(np.abs(d[:, ang] - h[:, ang]) / np.maximum(np.abs(h[:, ang]), np.finfo(float).tiny))
    gains = [(2 * L, L), (4 * L + 2 * Rk, Rk)]
    for off, cnt in gains:
        if cnt:
            gd, gh = d[:, off:off + 2 * cnt].reshape(-1, cnt, 2), h[:, off:off + 2 * cnt].reshape(-1, cnt, 2)
            mod = np.sqrt(np.sum(gh * gh, axis=2, keepdims=True))
            worst = max(worst, np.max(np.abs(gd - gh) / mod))
    print(f"{name}: paths worst {worst / EPS:.2f} eps")
    assert worst <= 16 * EPS


@pytest.mark.parametrize("name", MAIN)
def test_measurements_are_the_product_plus_the_mirrors_noise(gpu, name):
    """y against A vecH_device + noise_mirror (the product in extended precision): componentwise within the
    dot-product bound 8 (n + 16) eps sum_k |A_ik| |h_k| plus 16 eps times the noise modulus.  The device's own vecH
    keeps the channel's rounding out of the product's check."""
    from ace_amd import synth
    count, m, tx, rx, shared, _, _ = CASES[name]
    A, W = _inputs(name)
    d = _device(name)
    n = tx * rx
    worst = 0.0
    for c in range(count):
        Ac = A[0 if shared else c]
        h = d["vecH"][c]
        w = synth.scenario_noise(SEED, FIRST + c, m, rx, _cfg(name), W)
        ref = (Ac.astype(np.clongdouble) @ h.astype(np.clongdouble)) + w
        bound = 8 * (n + 16) * EPS * (np.abs(Ac) @ np.abs(h)) + 16 * EPS * np.abs(w)
        err = (d["y"][c] - ref).astype(np.complex128)
        worst = max(worst, np.max(np.maximum(np.abs(err.real), np.abs(err.imag)) / bound))
    print(f"{name}: y worst err / bound {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", MAIN)
def test_derived_outputs_follow_their_formulas_from_y(gpu, name):
    """y_noisy = y z (z the mirror's stream-12 draw; relative to the product's modulus), B_raw = |y|, B = B_raw /
    scale to 8 eps; scale = ||B_raw|| to (m + 8) eps."""
    from ace_amd import synth
    count, m = CASES[name][:2]
    d = _device(name)
    for c in range(count):
        z = synth.scenario_phase_noise(SEED, FIRST + c, m)
        yn = d["y"][c] * z
        assert np.all(np.abs(d["y_noisy"][c] - yn) <= 8 * EPS * np.abs(yn))
    B = np.abs(d["y"])
    assert np.all(np.abs(d["B_raw"] - B) <= 8 * EPS * B)
    sc = np.sqrt(np.sum(B.astype(np.longdouble) ** 2, axis=1)).astype(np.float64)
    assert np.all(np.abs(d["scale"] - sc) <= (m + 8) * EPS * sc)
    Bn = d["B_raw"] / d["scale"][:, None]
    assert np.all(np.abs(d["B"] - Bn) <= 8 * EPS * Bn)
    assert np.all(np.abs(np.sqrt(np.sum(d["B"] ** 2, axis=1)) - 1.0) <= (m + 16) * EPS)


@pytest.mark.parametrize("name", ["default_17x33", "default_3x256"])
def test_default_cfg_gives_synth_channels_outputs(gpu, name):
    """The default cfg against ace_synth_channels on the device.  The product's summation order differs (tiles on the
    matrix cores against one wave per probe), so bit-identity is not required."""
    import torch
    from ace_amd import synth_problem
    count, m, tx, rx = CASES[name][:4]
    A, _ = _inputs(name)
    _, B, X0, Hn = synth_problem(SEED, FIRST, count, m, tx, rx, A=torch.from_numpy(A).to("cuda:0"))
    torch.cuda.synchronize()
    d = _device(name)
    for k, ref in (("B", B), ("X0", X0), ("Hn", Hn)):
        assert np.allclose(d[k], ref.cpu().numpy(), rtol=1e-11, atol=1e-13), k
    h = _mirror(name)
    assert np.allclose(d["vecH"], h["vecH"], rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("name", ["rician_17x33", "combiner_3x9", "private_5x20"])
def test_a_realisation_does_not_depend_on_the_batch(gpu, name):
    """A one-realisation call at index first + c equals row c of the full call bit for bit (first, a middle and the
    last row; row 16 of the 17 sits alone in the second tile), on the default stream and on a side stream."""
    import torch
    from ace_amd.solver import Workspace
    count = CASES[name][0]
    full = _device(name)
    side, ws = torch.cuda.Stream(), Workspace()
    for c in (0, count // 2, count - 1):
        for stream in (None, side):
            torch.cuda.synchronize()
            one = _run(name, first=FIRST + c, count=1, rows=slice(c, c + 1), stream=stream,
                       workspace=None if stream is None else ws)
            for k in OUTS:
                assert np.array_equal(one[k][0], full[k][c]), (k, c, stream is not None)


def _raw_call(name, want):
    """ace_synth_scenario on buffers of its own: every output asked for lies between two guard regions of NaN; the
    others are NULL.  Returns ({output: array}, guards intact)."""
    import torch
    from ace_amd._lib import LIB, check
    count, m, tx, rx, shared, _, _ = CASES[name]
    from ace_amd.scenario import rician_in_effect
    cfg = _cfg(name)
    n, G = tx * rx, 64
    sizes = {"vecH": 2 * count * n, "y": 2 * count * m, "y_noisy": 2 * count * m, "B_raw": count * m, "scale": count,
             "B": count * m, "X0": 2 * count * n, "Hn": 2 * count * n, "paths": count * 4 * (cfg.L + rician_in_effect(cfg))}
    dev = torch.device("cuda:0")
    A, W = _inputs(name)
    Ad = torch.from_numpy(A).to(dev)
    Wd = None if W is None else torch.from_numpy(W).to(dev)
    bufs = {k: torch.full((sizes[k] + 2 * G,), float("nan"), dtype=torch.float64, device=dev) for k in want}
    Mr = 0 if W is None else W.shape[0]
    nb = int(LIB.ace_synth_scenario_workspace_size(C.byref(cfg), count, m, tx, rx, Mr))
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
    ptr = lambda k: bufs[k].data_ptr() + 8 * G if k in bufs else None   # noqa: E731
    check(LIB.ace_synth_scenario(C.byref(cfg), SEED, FIRST, count, m, tx, rx, Ad.data_ptr(), int(shared),
                                 None if Wd is None else Wd.data_ptr(), Mr, *[ptr(k) for k in OUTS], ws.data_ptr(),
                                 ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    out, ok = {}, True
    for k, b in bufs.items():
        h = b.cpu().numpy()
        ok = ok and bool(np.isnan(h[:G]).all() and np.isnan(h[-G:]).all())
        out[k] = h[G:-G]
    return out, ok


@pytest.mark.parametrize("name", ["rician_17x33", "private_5x20"])
def test_null_outputs_leave_the_others_bit_identical(gpu, name):
    full = _device(name)
    for want in (OUTS, ("y",), ("B",), ("X0", "paths"), ("scale", "y_noisy"), ("Hn",),
                 ("y", "y_noisy", "scale", "B", "X0", "Hn", "paths")):
        out, ok = _raw_call(name, want)
        assert ok, ("guard", want)
        for k in want:
            ref = full[k]
            ref = ref.view(np.float64) if np.iscomplexobj(ref) else ref
            assert np.array_equal(out[k], ref.reshape(-1)), (k, want)


def test_on_grid_paths_are_what_the_angle_estimate_reads(gpu):
    """L = 1 without NLOS paths and on_grid: the channel is one steering pair on the grid of angular.dictionary, so
    the strongest entry of the angular map is that grid point, and its angle is the one in ``paths``."""
    import torch
    from ace_amd import angular, scenario_batch, scenario_cfg, synth
    tx = rx = 8
    cfg = scenario_cfg(L=1, rician_k=0, on_grid=1)
    A = torch.from_numpy(synth.codebook(SEED, 9, tx * rx)).to("cuda:0")
    res = scenario_batch(SEED, 0, 24, tx, rx, A, cfg, want=("vecH", "paths"))
    aod, aoa, _, p, q = angular.estimate_angles(res.vecH, tx, rx)
    torch.cuda.synchronize()
    paths = res.paths.cpu().numpy()
    # the same grid points: index for index
    _, st, _ = angular.dictionary(tx)
    _, sr, _ = angular.dictionary(rx)
    assert np.array_equal(st[p.cpu().numpy()], synth._snap(np.sin(np.deg2rad(paths[:, 0])), 4 * tx))
    assert np.array_equal(sr[q.cpu().numpy()], synth._snap(np.sin(np.deg2rad(paths[:, 1])), 4 * rx))
    d = max(np.max(np.abs(aod.cpu().numpy() - paths[:, 0])), np.max(np.abs(aoa.cpu().numpy() - paths[:, 1])))
    print(f"on_grid: largest angle difference {d:.3g} deg")
    assert np.array_equal(aod.cpu().numpy(), paths[:, 0]) and np.array_equal(aoa.cpu().numpy(), paths[:, 1])
    assert len(np.unique(paths[:, 0])) > 4   # (several grid points are hit)


def test_a_zero_scale_gives_zeros_not_nan(gpu):
    """add_noise = 0 and a zero codebook: y = 0, scale = 0, and the three normalised outputs are zeros."""
    import torch
    from ace_amd import scenario_batch, scenario_cfg
    A = torch.zeros((1, 9, 16), dtype=torch.complex128, device="cuda:0")
    res = scenario_batch(SEED, 0, 3, 4, 4, A, scenario_cfg(add_noise=0))
    torch.cuda.synchronize()
    assert res.noise_power == 1e-10
    assert not res.scale.cpu().numpy().any() and not res.y.cpu().numpy().any()
    for k in ("B", "X0", "Hn"):
        v = getattr(res, k).cpu().numpy()
        assert np.isfinite(v).all() and not v.any(), k
    assert np.abs(res.vecH.cpu().numpy()).min() >= 0 and np.isfinite(res.vecH.cpu().numpy()).all()
