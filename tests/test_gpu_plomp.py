"""GPU tests of the sparse recoveries (ace_amd/sparse.py) and their sweep (montecarlo.vs_m_sparse) at 8 x 8
(n = 64, a 25 x 25 cut dictionary), M = 48, batch 8, with a short PhaseLift run: the tests are about the wiring (the
stages' own numerics are tested in test_gpu_phaselift.py and test_gpu_omp.py)."""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import omp_ref as OR  # noqa: E402

pytestmark = pytest.mark.gpu

TX = RX = 8
M, BATCH, SEED, S, PL_ITS = 48, 8, 21, 3, 40


def _up(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.fixture(scope="module")
def problem(gpu):
    from ace_amd import sparse
    from ace_amd.solver import synth_problem
    AD = sparse.dictionary_2d(TX, RX)[0]
    A, B, _, H = synth_problem(SEED, 0, BATCH, M, TX, RX, L=3, snr_db=30.0, device=gpu)
    ADd = _up(gpu, AD)
    return {"AD": AD, "ADd": ADd, "Phi": (A[0] @ ADd).contiguous(), "B": B, "H": H}


def test_plomp_batch_is_the_hand_composition(gpu, problem):
    import torch
    from ace_amd import sparse, omp_batch, phaselift_batch
    Phi, B, ADd = problem["Phi"], problem["B"], problem["ADd"]
    res = sparse.plomp_batch(Phi, B * B, S, maxIts=PL_ITS)
    ts = sparse.two_stage_setup(Phi.cpu().numpy(), S)
    assert 1 <= ts.mCS <= M and res.idx.shape == (BATCH, ts.mCS)
    sig = phaselift_batch(_up(gpu, ts.P), B * B, maxIts=PL_ITS).sig
    hand = omp_batch(_up(gpu, ts.C), sig, ts.mCS, 1e-12)
    for a, b in ((res.idx, hand.idx), (res.coef, hand.coef), (res.count, hand.count), (res.resnorm, hand.resnorm),
                 (res.status, hand.status)):
        assert torch.equal(a, b)
    Hh = res.channel(ADd).cpu().numpy()
    idx, coef = hand.idx.cpu().numpy(), hand.coef.cpu().numpy()
    for b in range(BATCH):
        k = int(hand.count[b])
        want = problem["AD"][:, idx[b, :k]] @ coef[b, :k]
        assert np.linalg.norm(Hh[b] - want) <= 1e-13 * max(1.0, np.linalg.norm(want))   # (AD[:, idx] @ coef)
    # the numpy form of channel() on the same numbers
    from ace_amd.omp import OmpResult
    hn = OmpResult(idx, coef, hand.count.cpu().numpy(), None, None, Phi.shape[1]).channel(problem["AD"])
    assert np.linalg.norm(hn - Hh) <= 1e-13 * np.linalg.norm(Hh)
    # max_atoms caps the OMP stage and leaves the first picks alone
    two = sparse.plomp_batch(Phi, B * B, S, max_atoms=2 * S, maxIts=PL_ITS)
    assert two.idx.shape == (BATCH, 2 * S)
    cnt = two.count.cpu().numpy()
    for b in range(BATCH):
        assert np.array_equal(two.idx[b, :cnt[b]].cpu().numpy(), idx[b, :cnt[b]])


def test_perfect_phase_cs_recovers_on_grid_channels(gpu, problem):
    """Noiseless channels of L = 3 well-separated grid columns, s = L: the support exactly, and the channel inside
    ||AD_I|| times the coefficient bound of tests/omp_ref.py (r = 0; doubled for the rounding of y = Phi c itself)."""
    from ace_amd import sparse
    AD, Phi = problem["AD"], problem["Phi"]
    Ph = Phi.cpu().numpy()
    rng = np.random.default_rng(4)
    Q = 25
    sups, gains = [], []
    for _ in range(BATCH):
        u = rng.permutation(3) * 10 + 1 + rng.integers(0, 3, 3)   # grid indices at least 8 steps (two beamwidths) apart
        v = rng.permutation(3) * 10 + 1 + rng.integers(0, 3, 3)
        sups.append(u * Q + v)
        gains.append(np.array([1.0, 0.8, 0.6]) * np.exp(2j * np.pi * rng.random(3)))
    Hn = np.stack([AD[:, s] @ g for s, g in zip(sups, gains)])
    Y = np.stack([Ph[:, s] @ g for s, g in zip(sups, gains)])
    res = sparse.perfect_phase_cs(Phi, _up(gpu, Y), S)
    idx, coef, cnt = res.idx.cpu().numpy(), res.coef.cpu().numpy(), res.count.cpu().numpy()
    Hr = res.channel(problem["ADd"]).cpu().numpy()
    for b in range(BATCH):
        assert cnt[b] == S and sorted(idx[b].tolist()) == sorted(sups[b].tolist()), b
        sv = np.linalg.svd(Ph[:, idx[b]], compute_uv=False)
        eps = 8.0 * (M + 2 * S + 2) * OR.U
        bound = np.linalg.norm(AD[:, idx[b]], 2) * 2 * eps * (sv[0] / sv[-1]) * (np.linalg.norm(gains[b]) + np.linalg.norm(Y[b]) / sv[0])
        err = np.linalg.norm(Hr[b] - Hn[b])
        print(f"perfect_phase_cs b={b}: kappa {sv[0] / sv[-1]:.2f}, err {err:.2e}, bound {bound:.2e}")
        assert err <= bound
    with pytest.raises(ValueError, match="m > 256"):
        import torch
        sparse.perfect_phase_cs(torch.zeros((257, 300), dtype=torch.complex128, device=gpu),
                                torch.zeros((1, 257), dtype=torch.complex128, device=gpu), 3)


def test_vs_m_sparse_composes_and_scores_vs_ms_channels(gpu):
    from ace_amd import evaluate_batch
    from ace_amd.montecarlo import vs_m_sparse, SPARSE
    from ace_amd.solver import synth_problem
    kw = dict(seed=SEED, pl_maxits=PL_ITS, chunk=4)
    full = vs_m_sparse(TX, RX, [M], 8, **kw)
    part = vs_m_sparse(TX, RX, [M], 3, first=2, **kw)   # rows 2 .. 4: the end of chunk 0 and the start of chunk 1
    keys = list(SPARSE) + [f"status_{k}" for k in SPARSE] + [f"count_{k}" for k in SPARSE] + ["gain_percsi_ana"]
    for k in keys:
        assert np.array_equal(part[k][:, :3], full[k][:, 2:5], equal_nan=True), k
    assert full["mCS"].tolist() == part["mCS"].tolist() and 1 <= full["mCS"][0] <= M and full["s"] == 3
    for k in SPARSE:
        assert full[k].shape == (1, 8, 4) and np.isfinite(full[k]).all()
        assert np.array_equal(full["mean"][k], full[k].mean(axis=1))
    assert (full["count_plomp"] <= full["mCS"][0]).all() and (full["count_perfect_cs"] == 3).all()
    assert np.array_equal(full["count_plomp_2s"], np.minimum(full["count_plomp"], 6))   # the same greedy path, capped
    # the H it scores is the one vs_m scores: synth_problem at (seed, chunk start, chunk, M), as vs_m_baselines reads it
    for c0 in (0, 4):
        H = synth_problem(SEED, c0, 4, M, TX, RX, L=3, snr_db=30.0, device=gpu)[3]
        assert np.array_equal(full["gain_percsi_ana"][0, c0:c0 + 4], evaluate_batch(H, H, TX, RX).gain_ana.cpu().numpy())
