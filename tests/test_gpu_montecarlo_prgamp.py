"""The PR-GAMP slot of the sparse Monte-Carlo sweep (ace_amd.montecarlo.vs_m_sparse(..., prgamp=True)): the new block
has finite metrics, and every other key equals the sweep without it bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_the_prgamp_slot_adds_its_block_and_changes_nothing_else(gpu):
    from ace_amd import montecarlo as MC
    kw = dict(seed=3, pl_maxits=60, device=gpu)
    a = MC.vs_m_sparse(16, 16, [64], 4, prgamp=True, max_try=2, **kw)
    b = MC.vs_m_sparse(16, 16, [64], 4, **kw)
    assert MC.SPARSE_PRGAMP == ("prgamp",)
    assert a["prgamp"].shape == (1, 4, 4) and np.isfinite(a["prgamp"]).all()
    assert a["status_prgamp"].shape == (1, 4) and a["tries_prgamp"].shape == (1, 4)
    # numTry is 1 .. max_try, or 0 where the reference would raise (MyPRGAMP's catch: zeros, ACE_ST_PRGAMP_FAILED) --
    # at this horizon the trajectories are chaotic, so which of the two a realisation does is not pinned here
    failed = (a["status_prgamp"] & 16384) != 0
    assert (a["tries_prgamp"][failed] == 0).all()
    assert ((a["tries_prgamp"][~failed] >= 1) & (a["tries_prgamp"][~failed] <= 2)).all()
    # (the evaluator's own bit, ACE_ST_EVAL_DEGENERATE, marks the zero channel of a failed realisation and nothing else)
    assert (((a["status_prgamp"] & 256) != 0) <= failed).all()
    assert np.isfinite(a["mean"]["prgamp"]).all()
    new = {"prgamp", "status_prgamp", "tries_prgamp"}
    assert set(a) - set(b) == new and set(b) <= set(a)
    for k, v in b.items():
        if k == "mean":
            assert set(a["mean"]) - set(v) == {"prgamp"}
            for kk, vv in v.items():
                assert np.array_equal(a["mean"][kk], vv, equal_nan=True), kk
        elif isinstance(v, np.ndarray):
            assert np.array_equal(a[k], v, equal_nan=True), k
        else:
            assert a[k] == v, k
