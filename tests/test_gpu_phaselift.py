"""GPU parity of the batched PhaseLift solver (ace_phaselift_solve_*) against the oracle.

Reference: main/src/my_recovery_algorithms/MyPhaseLift.m:69-107 with TFOCS solver_TraceLS /
tfocs_AT (oracle/tfocs_oracle.py, itself pinned by TFOCS's traceLS_problem1 known answer,
tests/test_oracle.py).  The GPU iterates in the reduced coordinates of range(Phi^H) (exact for
the zero start), so it differs from the dense oracle by rounding only.  TFOCS's backtracking
makes discrete decisions (|f_y - f_x| >= 1e-10 max(|f|), localL <= L) and the oracle is
rounding-sensitive against ITSELF beyond ~50-100 iterations (a 1e-15 input perturbation moves
the 8-antenna solution by 1e-5 at 100 iterations, 3e-3 at 200), so parity (1e-7, phase aligned)
is asserted on horizons where the oracle is stable against itself.
"""
import math

import numpy as np
import pytest

import ace_oracle as O
import tfocs_oracle as T

pytestmark = pytest.mark.gpu


def _problem(seed, tx, m, count):
    from ace_amd import synth
    n = tx * tx
    Phi = synth.codebook(seed, m, n) * math.sqrt(n)
    bs = []
    for r in range(count):
        h = synth.channel(seed, r, tx, tx)
        meas = np.abs(Phi @ h)
        meas = meas * 1.05 / np.sqrt(np.mean(meas ** 2))
        bs.append((meas / 2e5) ** 2 * 1e10)          # Recover_Channel.m:34 scaling
    return Phi, np.stack(bs)


@pytest.mark.parametrize("tx,m,its", [(8, 40, 40), (16, 121, 60), (4, 40, 40)])
def test_phaselift_short_horizon(gpu, tx, m, its):
    """(4, 40): m > n runs without the reduction (Q = I)."""
    from ace_amd import phaselift_host
    Phi, b = _problem(3 + tx, tx, m, 3)
    res = phaselift_host(Phi, b, maxIts=its)
    assert (res.iters == its).all()
    for r in range(3):
        sig, ref = T.my_phaselift(b[r], Phi, maxIts=its)
        assert ref.niter == its
        e = O.phase_aligned_rel_err(res.sig[r], sig)
        assert e <= 1e-6, (r, e)


def test_phaselift_tolerance_stop(gpu):
    """A loose tolerance stops the run early; the stopping iteration matches the oracle."""
    from ace_amd import phaselift_host, ACE_ST_CONVERGED
    Phi, b = _problem(5, 8, 40, 2)
    res = phaselift_host(Phi, b, maxIts=400, tol=2e-3)
    for r in range(2):
        sig, ref = T.my_phaselift(b[r], Phi, maxIts=400, tol=2e-3)
        assert ref.status.startswith("Step size")
        assert res.iters[r] == ref.niter and (res.status[r] & ACE_ST_CONVERGED)
        assert O.phase_aligned_rel_err(res.sig[r], sig) <= 1e-7


def test_phaselift_batch_invariance(gpu):
    from ace_amd import phaselift_host
    Phi, b = _problem(9, 8, 40, 4)
    full = phaselift_host(Phi, b, maxIts=120)
    for r in (0, 3):
        one = phaselift_host(Phi, b[r:r + 1], maxIts=120)
        assert np.array_equal(one.sig[0], full.sig[r]) and one.iters[0] == full.iters[r]


def test_myphaselift_signature(gpu):
    from ace_amd import MyPhaseLift, phaselift_host
    Phi, b = _problem(11, 8, 40, 1)
    x = MyPhaseLift(b[0][:, None], Phi, maxIts=30)
    assert x.shape == (64, 1)
    assert np.array_equal(x[:, 0], phaselift_host(Phi, b, maxIts=30).sig[0])


def test_phaselift_config4_geometry(gpu):
    """Config 4's geometry: 32 antennas (n = 1024, the lifted 1024 x 1024 PSD variable), m = 256
    measurements.  The oracle is the same TFOCS restatement in the coordinates of range(Phi^H)
    (tfocs_oracle.my_phaselift_reduced: the dense iteration up to rounding, pinned by
    test_oracle.py::test_phaselift_reduction_is_exact).  Against ITSELF with a 1e-15 input
    perturbation it moves 1.2e-12 at 60 iterations, 1.5e-10 at 80, 1e-6 at 120 and 7e-4 at 200
    (measured), so parity is asserted at 60 iterations (1e-8, phase aligned)."""
    from ace_amd import phaselift_host
    Phi, b = _problem(7, 32, 256, 3)
    res = phaselift_host(Phi, b, maxIts=60)
    assert (res.iters == 60).all()
    for r in range(3):
        sig, ref = T.my_phaselift_reduced(b[r], Phi, maxIts=60)
        assert ref.niter == 60
        e = O.phase_aligned_rel_err(res.sig[r], sig)
        assert e <= 1e-8, (r, e)


def test_phaselift_config4_batch_invariance_200(gpu):
    """The benchmarked horizon (200 TFOCS iterations) at config 4's geometry: a realisation's result
    in a 24-realisation batch is bit-identical to its result alone."""
    from ace_amd import phaselift_host
    Phi, b = _problem(13, 32, 256, 24)
    full = phaselift_host(Phi, b, maxIts=200)
    assert (full.iters == 200).all() and np.isfinite(full.sig).all()
    for r in (0, 23):
        one = phaselift_host(Phi, b[r:r + 1], maxIts=200)
        assert np.array_equal(one.sig[0], full.sig[r]) and one.iters[0] == full.iters[r]


def test_phaselift_config4_batch512_invariance(gpu):
    """The bench's batch (512 realisations, 200 TFOCS iterations): sampled realisations are
    bit-identical to their runs alone (the batch shares no arithmetic between realisations)."""
    from ace_amd import phaselift_host
    Phi, b = _problem(17, 32, 256, 512)
    full = phaselift_host(Phi, b, maxIts=200)
    assert (full.iters == 200).all() and np.isfinite(full.sig).all()
    for r in (0, 300, 511):
        one = phaselift_host(Phi, b[r:r + 1], maxIts=200)
        assert np.array_equal(one.sig[0], full.sig[r]) and one.iters[0] == full.iters[r], r



def test_phaselift_reduction_paths(gpu, monkeypatch):
    """The prox eig's reductions against each other at config 4's geometry: the unblocked and panel-blocked
    one-stage Householder reductions (hetrd_kernel, hetrd_blk_kernel; ACE_HETRD_BLK=0 / 1) and the two-stage
    one (ace_heev2.hip, the default; ACE_HETRD_BLK=2): the same iterations and solutions within 1e-9 at 60 TFOCS
    iterations (the oracle's own stable horizon), and each against the oracle (1e-8)."""
    from ace_amd import phaselift_host
    Phi, b = _problem(19, 32, 256, 4)
    res = {}
    for path in ("0", "1", "2"):
        monkeypatch.setenv("ACE_HETRD_BLK", path)
        res[path] = phaselift_host(Phi, b, maxIts=60)
    for path in ("1", "2"):
        assert np.array_equal(res[path].iters, res["0"].iters)
        for r in range(4):
            assert O.phase_aligned_rel_err(res[path].sig[r], res["0"].sig[r]) <= 1e-9, (path, r)
    sig, _ = T.my_phaselift_reduced(b[0], Phi, maxIts=60)
    for path in ("0", "1", "2"):
        assert O.phase_aligned_rel_err(res[path].sig[0], sig) <= 1e-8, path


def test_phaselift_order_512_takes_the_unblocked_fallback(gpu):
    """at d = m = 512 (32 antennas, 512 measurements; the reference's 32-antenna sweep reaches
    d = 841 and 1024) the blocked reduction's LDS exceeds the CU, and the solver must take the unblocked
    reduction instead of failing the solve with a refused launch (it used to record the refusal)."""
    from ace_amd import phaselift_host
    Phi, b = _problem(23, 32, 512, 2)
    res = phaselift_host(Phi, b, maxIts=8)
    assert (res.iters == 8).all() and np.isfinite(res.sig).all()
    for r in range(2):
        sig, ref = T.my_phaselift_reduced(b[r], Phi, maxIts=8)
        assert O.phase_aligned_rel_err(res.sig[r], sig) <= 1e-8, r


# ---------------------------------------------------------------- the branches no fixed-horizon solve above reaches
def _phase_problem(seed, tx, m, count, paths=2):
    """A random 2-bit-phase Phi (m x tx^2) and the scaled measurements of `count` sparse channels, from numpy seeds."""
    rng = np.random.default_rng([seed, tx, m])
    n = tx * tx
    Phi = (1j ** rng.integers(0, 4, (m, n))).astype(np.complex128)
    bs = []
    for _ in range(count):
        h = np.zeros(n, np.complex128)
        h[rng.choice(n, paths, replace=False)] = rng.standard_normal(paths) + 1j * rng.standard_normal(paths)
        meas = np.abs(Phi @ h)
        meas = meas * 1.05 / np.sqrt(np.mean(meas ** 2))
        bs.append((meas / 2e5) ** 2 * 1e10)
    return Phi, np.stack(bs)


def _oracle(b, Phi, lam=5e-2, **kw):
    """MyPhaseLift through tfocs_at_tracels with phaselift_ops (so that cntr_reset can be passed); also counts the
    prox calls with more than half of their eigenvalues above tau (the complement side's condition)."""
    n = Phi.shape[1]
    Aop, Aadj = T.phaselift_ops(Phi)
    stats = dict(calls=0, side=0)
    inner = T.prox_trace

    def counting(q, X, t):
        w = np.linalg.eigvalsh(0.5 * (X + X.conj().T))
        stats["calls"] += 1
        stats["side"] += int(2 * np.sum(w > q * t) > len(w))
        return inner(q, X, t)

    T.prox_trace = counting
    try:
        ref = T.tfocs_at_tracels(Aop, Aadj, b, lam, np.zeros((n, n), np.complex128), **kw)
    finally:
        T.prox_trace = inner
    w, V = np.linalg.eigh(ref.x)
    return math.sqrt(max(w[-1], 0.0)) * V[:, -1], ref, stats


@pytest.mark.parametrize("tx", [8, 4])
def test_phaselift_restart_and_exact_recomputation(gpu, tx):
    """restart = 15, cntr_reset = 3, 45 iterations at m = 40: the periodic restart of pl_iterate_kernel runs twice
    (iterations 15 and 30) and A_x / A_y are recomputed exactly every fourth step (need_Ay, need_Ax, the Aex
    branches).  tx = 4: m > n, the Q = I path.  The oracle against its own 1e-15 input perturbation moves (phase
    aligned, seeds as committed: 11 at tx = 8, 9 at tx = 4) 3.0e-13, 6.0e-12, 4.5e-13 at tx = 8 and 4.8e-14, 1.3e-14,
    3.2e-13 at tx = 4; over perturbations of 1e-15 to 1e-14 of either sign and two numpy / BLAS builds, at most
    1.1e-11 and 5.6e-13.  The figure depends on the build, because the oracle's backtracking decisions do: its final
    L differs by tens of percent between the two builds, and realisations of other seeds that move 1e-13 with one
    build move 1.5e-10 and 9.3e-10 with the other.  So the condition is asserted here, not assumed, and the seeds
    were chosen to hold it with a margin on both.  The GPU is held to max(1e-8, 100 x that distance) with equal
    iteration counts (measured: 5e-14 to 2.4e-12 from the oracle)."""
    from ace_amd import phaselift_host
    Phi, b = _phase_problem({8: 11, 4: 9}[tx], tx, 40, 3)
    kw = dict(maxIts=45, restart=15, cntr_reset=3)
    res = phaselift_host(Phi, b, **kw)
    for r in range(3):
        sig, ref, _ = _oracle(b[r], Phi, tol=1e-10, **kw)
        sigp, per, _ = _oracle(b[r] * (1 + 1e-15), Phi, tol=1e-10, **kw)
        dist = O.phase_aligned_rel_err(sigp, sig)
        assert ref.restarts >= 2 and ref.niter == per.niter == 45 and dist <= 1e-10, (r, ref.restarts, dist)
        assert res.iters[r] == ref.niter
        e = O.phase_aligned_rel_err(res.sig[r], sig)
        print(f"PL restart tx={tx} r={r}: oracle self-distance {dist:.2e}, GPU {e:.2e}")
        assert e <= max(1e-8, 100 * dist), (r, e, dist)


def test_phaselift_prox_side_matches_the_default(gpu, monkeypatch):
    """ACE_PROX_SIDE=1 (the prox from the eigenvectors at or below tau: the sign flip of pl_assemble_kernel and
    z = Zn + (W + W^H)/2 - tau I in pl_take_z_kernel) against the default: the same iterations, solutions within
    1e-9 at 45 iterations, each within 1e-8 of the oracle.  The solve does not report which side ran; on the oracle
    alone, about twenty of the ~49 prox calls of each realisation have more than half of their eigenvalues above
    tau (counted in the n = 64 coordinates, which implies it in the solve's d = 40)."""
    from ace_amd import phaselift_host
    Phi, b = _phase_problem(1, 8, 40, 3)
    monkeypatch.delenv("ACE_PROX_SIDE", raising=False)
    base = phaselift_host(Phi, b, maxIts=45)
    monkeypatch.setenv("ACE_PROX_SIDE", "1")
    side = phaselift_host(Phi, b, maxIts=45)
    assert np.array_equal(base.iters, side.iters)
    for r in range(3):
        sig, ref, stats = _oracle(b[r], Phi, maxIts=45, tol=1e-10, restart=200)
        assert stats["side"] >= 1 and ref.niter == 45 == base.iters[r], (r, stats)
        assert O.phase_aligned_rel_err(side.sig[r], base.sig[r]) <= 1e-9, r
        assert O.phase_aligned_rel_err(base.sig[r], sig) <= 1e-8 and O.phase_aligned_rel_err(side.sig[r], sig) <= 1e-8, r


def test_phaselift_batch_with_different_stopping_iterations(gpu):
    """A loose tolerance (2e-4) stops six realisations of one batch at six different iterations (the oracle's: 8,
    13, 6, 16, 7, 10); each is bit-identical to its run alone, with the oracle's iteration count: the done / act
    skipping of every kernel of the chain while the rest of the batch goes on."""
    from ace_amd import phaselift_host, ACE_ST_CONVERGED
    Phi, b = _phase_problem(2, 8, 40, 6)
    kw = dict(maxIts=400, tol=2e-4)
    want = []
    for r in range(6):
        _, ref, _ = _oracle(b[r], Phi, restart=200, **kw)
        assert ref.status.startswith("Step size")
        want.append(ref.niter)
    assert len(set(want)) >= 3, want
    full = phaselift_host(Phi, b, **kw)
    assert full.iters.tolist() == want and all(full.status & ACE_ST_CONVERGED)
    for r in range(6):
        one = phaselift_host(Phi, b[r:r + 1], **kw)
        assert one.iters[0] == want[r] and np.array_equal(one.sig[0], full.sig[r]), r
