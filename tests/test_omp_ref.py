"""CPU tests of the OMP reference (tests/omp_ref.py): its coefficients agree with numpy.linalg.lstsq on the chosen
supports, its trajectory is greedy, and EVERY realisation of every parity case of tests/test_gpu_omp.py meets the
four conditions under which a bit-different f64 implementation must pick the same atoms (none is left out)."""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import omp_ref as OR  # noqa: E402

CASES = [(s, w) for s in OR.SHAPES + [OR.TWO_STAGE] for w in (False, True)]
IDS = [("x".join(map(str, s)) if s != OR.TWO_STAGE else s) + ("-colscale" if w else "") for s, w in CASES]


@pytest.mark.parametrize("shape,scaled", CASES, ids=IDS)
def test_reference_against_lstsq_and_the_conditions(shape, scaled):
    c = OR.case(shape, scaled)
    D, Y, kmax = c["D"], c["Y"], c["kmax"]
    for mode, tol in (("count", 0.0), ("tol", OR.tol_for(c))):
        exp = OR.expected(c, tol)
        for b, e in enumerate(exp):
            k = e["count"]
            assert len(set(e["idx"])) == k and k <= kmax
            if k:
                ls = np.linalg.lstsq(D[:, e["idx"]], Y[b], rcond=None)[0]
                err = np.linalg.norm(ls - e["coef"].astype(np.complex128))
                assert err <= e["tol_coef"], (mode, b, err, e["tol_coef"])     # lstsq is itself a backward-stable QR
                rn = np.linalg.norm(Y[b] - D[:, e["idx"]] @ ls)
                assert abs(rn - float(e["resnorm"])) <= e["tol_res"]
            # stopped for a reason: the count is reached or the residual is within the tolerance, and not before
            assert k == kmax or e["resnorm"] <= tol
            assert all(c["traj"][b]["norms"][i] > tol for i in range(k))
        gap, rel, stop, kap = OR.conditions(c, tol)
        print(f"{shape} colscale={scaled} {mode}: min gap {gap:.2e}, min |r|/|y| {rel:.2e}, min stop gap {stop:.2e}, "
              f"max kappa {kap:.1f}, counts {sorted({e['count'] for e in exp})}")
        assert gap >= 1e-6 and rel >= 1e-6 and stop >= 1e-6 and kap <= 1e3
    if kmax > 1:   # the tolerance mode does stop some realisation early
        assert min(e["count"] for e in OR.expected(c, OR.tol_for(c))) < kmax


def test_residual_norms_decrease_and_the_f64_model_agrees():
    c = OR.case((33, 17, 130, 8), True)
    for b, t in enumerate(c["traj"]):
        assert all(t["norms"][i + 1] < t["norms"][i] for i in range(len(t["idx"])))
        m = OR.model(c["D"], c["Y"][b], c["kmax"], 0.0, c["w"])
        assert m["idx"] == t["idx"]
        assert np.linalg.norm(m["coef"] - t["coef"].astype(np.complex128)) <= OR.expected(c, 0.0)[b]["tol_coef"]


def test_ties_go_to_the_smaller_index_in_the_reference():
    rng = np.random.default_rng(1)
    D = OR._cn(rng, 6, 5)
    D[:, 3] = D[:, 1]
    y = 2.0 * D[:, 1] + 0.1 * D[:, 4]
    t = OR.model(D, y, 2, dtype=OR.CLD)
    assert t["idx"][0] == 1 and 3 not in t["idx"]
