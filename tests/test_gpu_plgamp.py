"""GPU tests of the PLGAMP wiring (sparse.plgamp_batch, sparse.two_stage_batch, montecarlo.vs_m_sparse(gamp=True)) and
of the directional driver (engine.recover_directional) at 16 x 16 with a short PhaseLift run: the tests are about the
composition (the stages' own numerics are tested in test_gpu_phaselift.py, test_gpu_omp.py and test_gpu_gamp.py)."""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
from make_directional_golden import unpack  # noqa: E402

pytestmark = pytest.mark.gpu

TX = RX = 16
M, BATCH, SEED, S, PL_ITS = 36, 4, 21, 3, 200


def _up(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.fixture(scope="module")
def problem(gpu):
    from ace_amd import sparse
    from ace_amd.solver import synth_problem
    ADd = _up(gpu, sparse.dictionary_2d(TX, RX)[0])
    A, B, _, H = synth_problem(SEED, 0, BATCH, M, TX, RX, L=3, snr_db=30.0, device=gpu)
    return {"ADd": ADd, "Phi": (A[0] @ ADd).contiguous(), "B": B}


def test_plgamp_batch_is_the_hand_composition_and_carries_the_omp_fallback(gpu, problem):
    import torch
    from ace_amd import sparse, embgamp_batch, omp_batch, ACE_ST_GAMP_FAILED
    Phi, B = problem["Phi"], problem["B"]
    n = Phi.shape[1]
    meas = (B * B).clone()
    meas[2] = meas[2] * 1e100          # an intermediate vector of about 1e49: EMBGAMP leaves through its failure path
    res = sparse.plgamp_batch(Phi, meas, S, 1.0, maxIts=PL_ITS)
    ts, sig = sparse.plomp_stage1(Phi, meas, S, maxIts=PL_ITS)
    hand = embgamp_batch(ts.C, sig, 0.0, S / n)
    fb = omp_batch(ts.C, sig, ts.mCS, 1e-12, want_x=True)
    st = res.status.cpu().numpy().view(np.uint32)
    assert torch.equal(res.status, hand.status) and torch.equal(res.em_iters, hand.em_iters)
    assert [bool(v & ACE_ST_GAMP_FAILED) for v in st] == [False, False, True, False]
    for b in range(BATCH):
        want = fb.x[b] if st[b] & ACE_ST_GAMP_FAILED else hand.xhat[b]
        assert torch.equal(res.xhat[b], want), b
    assert res.xhat.shape == (BATCH, n) and bool(torch.isfinite(torch.view_as_real(res.xhat)).all())
    H = res.channel(problem["ADd"])
    assert H.shape == (BATCH, TX * RX)
    assert torch.allclose(H, res.xhat @ problem["ADd"].T, rtol=1e-12, atol=1e-12)


def test_two_stage_batch_returns_both_methods_of_one_phaselift_run(gpu, problem):
    import torch
    from ace_amd import sparse
    Phi, B = problem["Phi"], problem["B"]
    omp, gamp = sparse.two_stage_batch(Phi, B * B, S, 1.0, maxIts=PL_ITS)
    plomp = sparse.plomp_batch(Phi, B * B, S, maxIts=PL_ITS)
    for a, b in ((omp.idx, plomp.idx), (omp.coef, plomp.coef), (omp.count, plomp.count), (omp.resnorm, plomp.resnorm),
                 (omp.status, plomp.status)):
        assert torch.equal(a, b)
    plgamp = sparse.plgamp_batch(Phi, B * B, S, 1.0, maxIts=PL_ITS)
    assert torch.equal(gamp.xhat, plgamp.xhat) and torch.equal(gamp.status, plgamp.status)


def test_vs_m_sparse_with_gamp_adds_keys_and_leaves_the_old_ones_alone(gpu):
    from ace_amd.montecarlo import vs_m_sparse, SPARSE, SPARSE_GAMP
    kw = dict(seed=SEED, pl_maxits=40, chunk=4)
    old = vs_m_sparse(8, 8, [48], 4, **kw)
    new = vs_m_sparse(8, 8, [48], 4, gamp=True, **kw)
    assert not any(k in old or f"status_{k}" in old for k in SPARSE_GAMP)
    for k in old:
        if k in ("mean", "columns"):
            continue
        assert np.array_equal(old[k], new[k], equal_nan=True), k
    for k in SPARSE:
        assert np.array_equal(old["mean"][k], new["mean"][k])
    for k in SPARSE_GAMP:
        assert new[k].shape == (1, 4, 4) and np.isfinite(new[k]).all(), k
        assert new[f"status_{k}"].shape == (1, 4) and new[f"em_iters_{k}"].shape == (1, 4)
        assert (new[f"em_iters_{k}"] >= 1).all() and np.array_equal(new["mean"][k], new[k].mean(axis=1))


def test_the_directional_driver(gpu):
    """16 x 16 on the reference's directional codebook (the fixture), rss from the project's synth,
    10 log10(1000 (|beams h| / rss_fct)^2): the shapes, and each slot against its method composed by hand."""
    from ace_amd import engine, sparse, synth
    cb = unpack()
    n = TX * RX
    assert cb.shape == (32, 32, n)
    h = synth.channel(SEED, 0, TX, RX, 3)
    rss = 10.0 * np.log10(1000.0 * (np.abs(cb @ h) / engine.RSS_FCT) ** 2)
    Ms = [2, 6]
    amp, ang = engine.recover_directional(TX, RX, np.abs(cb), np.angle(cb), rss, 3, Mt_list=Ms, pl_maxits=PL_ITS)
    assert amp.shape == ang.shape == (2, 2, n)
    assert np.isfinite(amp).all() and np.isfinite(ang).all() and (amp >= 0).all()
    AD = _up(gpu, sparse.dictionary_2d(TX, RX, 4 * TX, 4 * RX, 180.0, 2.9e-3)[0])
    assert AD.shape == (n, 16 * n)
    cb = np.abs(cb) * np.exp(1j * np.angle(cb))   # as the driver rebuilds it (:128), rounding of exp included
    for i, Mc in enumerate(Ms):
        idx = np.floor(np.linspace(1.0, 32.0, Mc) + 0.5).astype(np.int64) - 1
        beams = np.stack([cb[idx[p % Mc], idx[p // Mc]] for p in range(Mc * Mc)])     # row i + M j of MATLAB's reshape
        meas = np.sqrt(10.0 ** (np.array([rss[idx[p % Mc], idx[p // Mc]] for p in range(Mc * Mc)]) / 10.0) / 1000.0) * engine.RSS_FCT
        msq = _up(gpu, ((meas / 2e5) ** 2 * 1e10)[None, :])
        Phi = (_up(gpu, beams) @ AD).contiguous()
        hands = (sparse.plomp_batch(Phi, msq, 3, maxIts=PL_ITS), sparse.plgamp_batch(Phi, msq, 3, 1.0, maxIts=PL_ITS))
        for slot, r in enumerate(hands):
            Hh = r.channel(AD)[0].cpu().numpy() / np.sqrt(1e10) * 2e5 / engine.RSS_FCT
            Hh[np.isnan(Hh)] = 0
            assert np.array_equal(amp[i, slot], np.abs(Hh)) and np.array_equal(ang[i, slot], np.angle(Hh)), (Mc, slot)
    eng = engine.start_matlab()
    assert engine.directional_sweep(16, 16).tolist() == [2, 6, 11, 15, 19, 23, 28, 32]
    assert engine.directional_sweep(32, 32).tolist() == [2, 11, 20, 29, 37, 46, 55, 64]
    with pytest.raises(ValueError, match="sweep point 1: M = 40"):
        engine.recover_directional(TX, RX, np.abs(cb), np.angle(cb), rss, 3, Mt_list=[2, 40], pl_maxits=PL_ITS)
    with pytest.raises(engine.MatlabExecutionError):
        eng.channel_recovery_ADMM_v2_simulation_directional(TX, RX, np.abs(cb), np.angle(cb), rss, 3, nargout=1)
    with pytest.raises(engine.MatlabExecutionError):
        engine.recover_directional(TX, RX, np.abs(cb)[:8], np.angle(cb)[:8], rss, 3)
