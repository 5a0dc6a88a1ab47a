"""The numpy oracle of the min-L2 tests (tests/minl2_ref.py) against what inferMinL2.m implies.  No GPU.

  * m_t <= n with full row rank: A pinv(A) = I, so the first iteration already has |Y| = B, J_M = 0, and the stage stops
    after one iteration with X = pinv(A) normalize_rows(A X0);
  * the column-count block that stands twice in the file is idempotent on every generated case;
  * the float64, the long-double and the row-permuted float64 runs agree in every decision (iters, objcol, the mu
    schedule) on at least 7 of 8 realisations per shape and mode -- the condition under which tests/test_gpu_minl2.py
    compares the kernel exactly -- in the row form at full length and in the other forms capped at 40 iterations;
  * the recovery works: at n = 16, m = 64, 30 dB the median NMSE over 8 draws is below 0.05."""
import numpy as np
import pytest

import minl2_ref as R

CHEAP = ((5, 17), (16, 48), (20, 17))


@pytest.mark.parametrize("sbr", [True, False])
def test_m_le_n_stops_after_one_iteration(sbr):
    A, B, X0, _ = R.problem(20, 17)
    for b in range(R.NB):
        for dt in (np.float64, np.longdouble):
            o = R.infer_admm(A, B[b], X0[b].T, sbr, dt)
            assert o["iters"] == 1 and o["converged"]
            AX = A @ X0[b].T
            sc = np.linalg.norm(B[b]) / (np.linalg.norm(AX) if sbr else np.linalg.norm(AX, axis=0))
            want = np.linalg.pinv(A) @ R.normalize_rows(AX * sc, B[b], sbr)
            assert np.linalg.norm(np.asarray(o["Xall"], complex) - want) <= 1e-12 * np.linalg.norm(want)
            assert float(o["opt_obj"]) <= 64 * 17 * R.U64 * np.linalg.norm(B[b])


def test_the_duplicated_column_count_block_is_idempotent():
    seen = set()
    for n, m in R.SHAPES + ((4, 16), (16, 64), (33, 100), (64, 61)):
        A, B, _, _ = R.problem(n, m)
        for b in range(R.NB):
            X, (r1, r2) = R.spectral_init(A, B[b], min(20, m, n))
            assert r1 == r2 == X.shape[1] and 1 <= r2 <= min(20, m, n)
            seen.add((n, r2))
    assert any(n == 16 and r < 16 for n, r in seen)      # the rule fires at n = 16 ...
    assert all(r == 20 for n, r in seen if n >= 33)       # ... and leaves r = 20 from n = 33 on


# (m <= n in the per-column form is left out: every objective is at rounding level, the best column rounding noise)
@pytest.mark.parametrize("n,m,mode", [(n, m, mode) for n, m in CHEAP for mode in ("row", "col40", "r1_40")
                                      if (n, m, mode) != (20, 17, "col40")])
def test_precisions_agree(n, m, mode):
    c = R.stage_case(n, m, mode)
    assert sum(c["counts"]) >= 7, c["counts"]
    for b in range(R.NB):
        if c["counts"][b]:
            ref = c["ref"][b]
            assert c["spread"][b]["Xall"] <= 1e-5 * float(np.linalg.norm(np.asarray(ref["Xall"], complex)))


def test_5x17_per_column_at_full_length_agrees():
    assert sum(R.stage_case(5, 17, "col")["counts"]) >= 7


def test_the_recovery_works_at_16x64():
    A, B, _, x = R.problem(16, 64)
    tr = np.random.default_rng(3).permutation(64)[:61]
    nm = []
    for b in range(R.NB):
        X, _, q, info = R.infer_min_l2(A, B[b], tr)
        a = np.vdot(X, x[b]) / np.vdot(X, X)
        nm.append(np.linalg.norm(a * X - x[b]) ** 2 / np.linalg.norm(x[b]) ** 2)
        assert info["r_used"] < 16 and q > 0.6
    print("NMSE per draw:", " ".join(f"{v:.4f}" for v in nm))
    assert np.median(nm) < 0.05
