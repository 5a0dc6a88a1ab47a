"""The Vs_M sweep of the recovery without a prior (montecarlo.vs_m_minl2): shards reproduce the full run bit for
bit, and more measurements recover better."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_shards_compose_and_more_measurements_help(gpu):
    from ace_amd import montecarlo
    full = montecarlo.vs_m_minl2(4, 4, [16, 64], 8, seed=3, chunk=4)
    a = montecarlo.vs_m_minl2(4, 4, [16, 64], 4, seed=3, chunk=4, first=0)
    b = montecarlo.vs_m_minl2(4, 4, [16, 64], 4, seed=3, chunk=4, first=4)
    for k in ("metrics", "status", "r_used", "quality", "stage_iters"):
        assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), full[k], equal_nan=True), k
    assert set(full) == {"M", "metrics", "status", "mean", "n_degenerate", "columns",   # vs_m's keys ...
                         "r_used", "quality", "stage_iters"}
    assert full["metrics"].shape == (2, 8, 4) and full["r_used"].shape == (2, 8)
    assert np.isnan(full["quality"][0]).all() and (full["quality"][1] == full["quality"][1]).all()   # M = 16: no test rows
    nmse = full["mean"][:, full["columns"].index("nmse")]
    print("vs_m_minl2 4x4: mean NMSE at M = 16, 64:", nmse)
    assert nmse[1] < nmse[0]
